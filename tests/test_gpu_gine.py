"""GINEConv with edge features on the HIP path (csrc/gine.hip) against the plain-torch restatement of
tests/gine_oracle.py.

Tolerances are the project's own (tests/helpers.py), no new constants:
  * the forward aggregate z by ``check_f64``: |z - z64| <= 3 n 2^-24 mag with n = deg_i + De + 4 and
    mag = (1+eps)|x_i| + sum_k (|x_src| + |W||e_k| + |b|), and the same bound must REJECT z64 with the largest single
    message removed;
  * every gradient by ``referee_all`` (float32 and float64 restatements as the two oracles) with ``teeth``: the float64
    run with one edge removed must be rejected.

Gate condition, asserted with no exclusion: every ReLU input of the float64 restatement lies farther from zero than
4 x the forward bound of its tensor, so that no gate can differ between HIP, float32 and float64.  For the operator
cases the bound is a-priori and taken element by element (``_gate_bounds``): 3 (De + 2) 2^-24 (|x_src| + |W||e| + |b|)
for a message's pre-activation, 3 (deg_i + De + 4 + F + 1) 2^-24 (mag_z |W0|^T + |b0|) for the MLP's hidden layer (the
bound of z carried through the first Linear, plus that Linear's own sum of F + 1 terms).  Through three
stacked layers on integer atom features the same form over absolute values grows to ~1e-1 and says nothing, so for
the model case the bound of a tensor is the referee's own limit for it, from the reference's own error:
2 max|f32 - f64| + 8 2^-23 max|f64| (the bar the prediction is held to).  The seeds below were chosen on the CPU so
that the guards hold."""
import copy

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT
from graph_hscn.data import Batch, DataLoader
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.mpnn import MPNN
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GINE
from graph_hscn.structure import Relation
from tests import gine_oracle as GO
from tests.helpers import DEV, F64_C, U32, KinkGuard, check_f64, f64_close, grads_of, most_changed, referee_all, teeth

pytestmark = pytest.mark.gpu

LONG, CHUNK = Fh.GINE_LONG_ROW, Fh.GINE_CHUNK


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def _multigraph(N, E, seed):
    """[2, E] in RANDOM edge order (so that the CSR's eid[slot] != slot): the last four nodes are isolated, nodes 1 and
    2 carry a self loop each, the first two random edges occur three times."""
    g = torch.Generator().manual_seed(seed)
    live = max(N - 4, 1)
    base = torch.randint(0, live, (2, E - 6), generator=g)
    extra = torch.tensor([[1 % live, 2 % live], [1 % live, 2 % live]])
    ei = torch.cat([base, extra, base[:, :2], base[:, :2]], 1)
    return ei[:, torch.randperm(E, generator=g)].contiguous()


def _inputs(N, E, F, De, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(N, F, generator=g)
    ea = torch.randn(E, De, generator=g)
    W = torch.randn(F, De, generator=g) / De ** 0.5
    b = 0.1 * torch.randn(F, generator=g)
    return x, ea, W, b


def _hip_aggregate(x, ei, ea, W, b, eps, rel=None):
    N = x.size(0)
    rel = rel if rel is not None else Relation(ei.to(DEV), N, N)
    return Fh.GINEAggregateFn.apply(x.to(DEV), ea.to(DEV), W.to(DEV), b.to(DEV), rel, eps), rel


def _largest_message(x, ei, ea, W, b):
    m = torch.relu(GO.pre_activations(x.double(), ei, ea.double(), W.double(), b.double()))
    return int(m.max(1).values.argmax())


def _check_forward(x, ei, ea, W, b, eps, what, wrong_rows=False):
    z, rel = _hip_aggregate(x, ei, ea, W, b, eps)
    d = (x.double(), ei, ea.double(), W.double(), b.double())
    z64 = GO.aggregate(*d, eps=eps)
    mag, n = GO.aggregate_magnitude(*d, eps=eps)
    if ei.size(1) == 0:
        assert f64_close(z, z64, mag, n, what=what), what
        return z
    dropped = GO.aggregate(*d, eps=eps, skip=_largest_message(x, ei, ea, W, b))
    check_f64(z, z64, mag, n, dropped, what=what)
    if wrong_rows:      # the edge-feature row of a CSR slot is edge_attr[eid[slot]]: taking edge_attr[slot] must fail
        slot_edge = torch.argsort(ei[1], stable=True)
        assert not torch.equal(slot_edge, torch.arange(ei.size(1)))
        ea_slot = torch.empty_like(ea)
        ea_slot[slot_edge] = ea
        z_slot = GO.aggregate(x.double(), ei, ea_slot.double(), W.double(), b.double(), eps=eps)
        assert not f64_close(z, z_slot, mag, n), f"{what}: the bound cannot tell eid[slot] from slot"
    assert int(rel.csr.flag.item()) == 0
    return z


# --------------------------------------------------------------------------- #
# 1. forward
# --------------------------------------------------------------------------- #
# F x De: the kernel branches on F % 4 (16-byte or scalar lanes), on the lanes per row (F = 68: 17 lanes, a block with
# idle lanes at its end; F = 70 / 260: more than 64 lanes' worth, a second column pass -- added to the issue's list) and on
# De <= 4 / <= 8 / above (weights in 4 or 8 registers per column, or read per edge).  De = 1 and De = 3 take the same
# branch and differ in how many of the four register columns are live: De = 1 runs at F in {1, 16, 33} only (one
# width per lane shape); every other combination of the issue's table runs.
_WIDTHS = [1, 3, 9, 16, 17, 33, 64, 68]
FORWARD_CASES = ([(F, De) for F in _WIDTHS for De in (3, 7, 16)] + [(F, 1) for F in (1, 16, 33)]
                 + [(70, 3), (260, 3), (260, 16)])


@pytest.mark.parametrize("F,De", FORWARD_CASES)
def test_forward_matches_float64_at_every_width_and_edge_dim(F, De):
    N, E = 64, 400
    ei = _multigraph(N, E, seed=F * 100 + De)
    deg = torch.bincount(ei[1], minlength=N)
    assert int((deg == 0).sum()) >= 4 and bool((ei[0] == ei[1]).any())
    assert torch.unique(ei[0] * N + ei[1]).numel() < E                     # repeated edges
    x, ea, W, b = _inputs(N, E, F, De, seed=F + De)
    _check_forward(x, ei, ea, W, b, 0.0, f"GINE forward F={F} De={De}", wrong_rows=True)


def test_forward_without_edges_on_one_node_and_with_eps():
    x, ea, W, b = _inputs(7, 0, 9, 3, seed=1)
    z = _check_forward(x, torch.zeros(2, 0, dtype=torch.int64), ea, W, b, 0.25, "GINE forward E=0")
    assert torch.equal(z.cpu(), (1.25 * x))                                # exact: one rounding, no sum
    x, ea, W, b = _inputs(1, 3, 16, 3, seed=2)
    _check_forward(x, torch.zeros(2, 3, dtype=torch.int64), ea, W, b, 0.0, "GINE forward N=1 (three loops)")
    ei = _multigraph(64, 400, seed=5)
    x, ea, W, b = _inputs(64, 400, 17, 7, seed=3)
    z0 = _check_forward(x, ei, ea, W, b, 0.0, "GINE forward eps=0")
    z1 = _check_forward(x, ei, ea, W, b, 0.25, "GINE forward eps=0.25", wrong_rows=True)
    assert not torch.equal(z0, z1)


# --------------------------------------------------------------------------- #
# gradients of the layer: referee, teeth, gate condition
# --------------------------------------------------------------------------- #
def _pre_bound(x, ei, ea, W, b):
    """[E, F]: the a-priori forward bound of every message pre-activation (module docstring)."""
    mag_pre = GO.pre_activations(x.double().abs(), ei, ea.double().abs(), W.double().abs(), b.double().abs())
    return F64_C * (W.shape[1] + 2) * U32 * mag_pre


def _gate_bounds(x, ei, ea, ref64):
    """A-priori forward bounds (module docstring) of the two gated tensors of one layer, element by element."""
    W, b = ref64.lin.weight.detach(), ref64.lin.bias.detach()
    mag_z, n_z = GO.aggregate_magnitude(x.double(), ei, ea.double(), W, b, float(ref64.eps))
    W0, b0 = ref64.nn[0].weight.detach(), ref64.nn[0].bias.detach()
    mag_h = mag_z @ W0.abs().t() + b0.abs()
    return {"message pre-activation": _pre_bound(x, ei, ea, W, b),
            "MLP hidden layer": F64_C * (n_z + W.shape[0] + 1) * U32 * mag_h}


def _check_gates(guards, bounds, what):
    """Every watched ReLU input farther from zero than 4 x its own bound: the guard sees |v| / bound against 1."""
    for tag, seen in guards.items():
        kg = KinkGuard()
        for v in seen:
            kg.watch(tag, v.double() / bounds[tag])
        kg.check(1.0, what=f"{what} {tag} (in units of its forward bound)")


def _ref_step(ref32, x, ei, ea, gy, dtype, skip=None, guards=None):
    m = copy.deepcopy(ref32).to(dtype)
    m.watch = None if guards is None else (lambda tag, t: guards[tag].append(t.detach()))
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    out = m(xx, ei, ea.to(dtype), skip)
    out.backward(gy.to(dtype))
    g = {"x.x": xx.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    return g, out.detach()


def _layer_shape(F):
    """(N, E) of a layer case: the smallest multigraph with every structure of ``_multigraph``; at 64 columns fewer
    nodes, so that a seed can meet the gate condition on all N x H hidden inputs."""
    return (40, 90) if F < 64 else (16, 40)


def _layer_case(N, E, F, H, De, seed, ei=None, device=DEV):
    """Product layer and restatement with identical weights, and the inputs."""
    torch.manual_seed(seed)
    ref = GO.gine_layer(F, H, De)
    prod = GINE(F, H, edge_dim=De).to(device)
    GO.copy_weights(ref, prod)
    ei = _multigraph(N, E, seed) if ei is None else ei
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(N, F, generator=g)
    ea = torch.randn(ei.size(1), De, generator=g)
    gy = torch.randn(N, H, generator=g)
    return ref, prod, ei, x, ea, gy


def _referee_layer(ref, prod, ei, x, ea, gy, what):
    guards = {"message pre-activation": [], "MLP hidden layer": []}
    o32, out32 = _ref_step(ref, x, ei, ea, gy, torch.float32)
    o64, out64 = _ref_step(ref, x, ei, ea, gy, torch.float64, guards=guards)
    _check_gates(guards, _gate_bounds(x, ei, ea, copy.deepcopy(ref).double()), what)
    skip = _largest_message(x, ei, ea, ref.lin.weight.detach(), ref.lin.bias.detach())
    d64, dout64 = _ref_step(ref, x, ei, ea, gy, torch.float64, skip=skip)
    xd = x.to(DEV).requires_grad_(True)
    prod.zero_grad(set_to_none=True)
    out = prod(xd, ei.to(DEV), ea.to(DEV))
    out.backward(gy.to(DEV))
    got = grads_of(prod, x=xd)
    referee_all({"out": out}, {"out": out32}, {"out": out64}, what)
    teeth({"out": out}, {"out": out32}, {"out": out64}, {"out": dout64}, what)
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    assert {"x.x", "p.lin.weight", "p.lin.bias", "p.nn.0.weight", "p.nn.2.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what)
    return got, xd


# (F, H, De) -> seed whose float64 run satisfies the gate condition (chosen on the CPU; asserted in the test)
BACKWARD_SEEDS = {(9, 16, 3): 1, (9, 16, 7): 1, (16, 16, 3): 1, (16, 16, 7): 2,
                  (17, 10, 3): 2, (17, 10, 7): 1, (64, 64, 3): 8, (64, 64, 7): 5}


@pytest.mark.parametrize("F,H,De", sorted(BACKWARD_SEEDS))
def test_backward_of_every_leaf(F, H, De):
    N, E = _layer_shape(F)
    ref, prod, ei, x, ea, gy = _layer_case(N, E, F, H, De, BACKWARD_SEEDS[(F, H, De)])
    what = f"GINE layer F={F} H={H} De={De}"
    got, xd = _referee_layer(ref, prod, ei, x, ea, gy, what)
    assert set(got) == {"x.x", "p.lin.weight", "p.lin.bias", "p.nn.0.weight", "p.nn.0.bias", "p.nn.2.weight",
                        "p.nn.2.bias"}
    # a second backward on the same inputs: the same bits
    prod.zero_grad(set_to_none=True)
    xd2 = x.to(DEV).requires_grad_(True)
    prod(xd2, ei.to(DEV), ea.to(DEV)).backward(gy.to(DEV))
    again = grads_of(prod, x=xd2)
    for k in got:
        assert torch.equal(again[k], got[k]), k
    # x without a gradient (the first layer of a model): no gx, the parameter gradients unchanged bit for bit
    prod.zero_grad(set_to_none=True)
    x3 = x.to(DEV)
    z = prod.aggregate(x3, ei.to(DEV), ea.to(DEV))
    assert z.grad_fn.next_functions[0][0] is None            # no edge of the autograd graph towards x
    prod.nn[2](prod.nn[0](z, act="relu")).backward(gy.to(DEV))
    assert x3.grad is None
    for k, v in grads_of(prod).items():
        assert torch.equal(v, got[k]), k
    with pytest.raises(NotImplementedError, match="edge_attr"):
        prod(xd, ei.to(DEV), ea.to(DEV).requires_grad_(True))


# --------------------------------------------------------------------------- #
# 2. long rows: the whole-block path of the forward (in-degree) and of the backward's source walk (out-degree)
# --------------------------------------------------------------------------- #
def _hub_graph(N, d, seed):
    """Node 0 receives ``d`` edges and node 1 sends ``d`` (repeated edges from / to the other nodes), plus 2 N random
    edges; random edge order."""
    g = torch.Generator().manual_seed(seed)
    others = torch.arange(d) % (N - 2) + 2
    ei = torch.cat([torch.stack([others, torch.zeros(d, dtype=torch.int64)]),
                    torch.stack([torch.ones(d, dtype=torch.int64), others]),
                    torch.randint(2, N, (2, 2 * N), generator=g)], 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


# one below, at and one above the split threshold; the same around a chunk boundary inside a split row; 3 x the threshold
HUB_DEGREES = [LONG - 1, LONG, LONG + 1, LONG + CHUNK - 1, LONG + CHUNK, LONG + CHUNK + 1, 3 * LONG]
HUB_N, HUB_DE = 24, 3


def _hub_inputs(F, d, seed):
    ei = _hub_graph(HUB_N, d, seed=d)
    indeg, outdeg = torch.bincount(ei[1], minlength=HUB_N), torch.bincount(ei[0], minlength=HUB_N)
    assert int(indeg[0]) == d and int(outdeg[1]) == d
    assert int(indeg[1:].max()) < LONG - 1 and int(outdeg[0]) < LONG - 1 and int(outdeg[2:].max()) < LONG - 1
    return (ei,) + _inputs(HUB_N, ei.size(1), F, HUB_DE, seed)


# widths: 16 (4 lanes per row: 64 lane groups, every chunk of a row in one round), 17 (scalar lanes, 15 lane groups
# and idle lanes at the end of the block), 256 (64 lanes per row: 4 lane groups, so LONG + 1 slots already take a second
# round of chunks)
@pytest.mark.parametrize("F", [16, 17, 256])
@pytest.mark.parametrize("d", HUB_DEGREES)
def test_long_rows_forward(F, d):
    ei, x, ea, W, b = _hub_inputs(F, d, seed=F + d)
    _check_forward(x, ei, ea, W, b, 0.0, f"GINE hub forward d={d} F={F}", wrong_rows=True)


def _aggregate_grads(x, ei, ea, W, b, gz, dtype, skip=None, seen=None):
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (x, W, b)]
    z = GO.aggregate(leaves[0], ei, ea.to(dtype), leaves[1], leaves[2], 0.0, skip,
                     None if seen is None else (lambda tag, t: seen.append(t.detach())))
    z.backward(gz.to(dtype))
    return dict(zip(("x.x", "x.W", "x.b"), (t.grad.detach().clone() for t in leaves)))


# (F, d) -> seed whose float64 pre-activations satisfy the gate condition (chosen on the CPU; asserted in the test).
# The source walk at 128 columns has 8 lane groups: 3 x LONG slots take two rounds of chunks there.
HUB_GX_SEEDS = {(F, d): 0 for F in (16, 17, 128) for d in HUB_DEGREES}
HUB_GX_SEEDS.update({(16, LONG + CHUNK + 1): 1, (16, 3 * LONG): 1, (128, LONG + 1): 1, (128, 3 * LONG): 1})


@pytest.mark.parametrize("F,d", sorted(HUB_GX_SEEDS))
def test_long_rows_gx(F, d):
    """gx (and the gradients of lin, through gm) with a node of out-degree ``d``: the source walk's long-row path."""
    ei, x, ea, W, b = _hub_inputs(F, d, seed=HUB_GX_SEEDS[(F, d)])
    gz = torch.randn(HUB_N, F, generator=torch.Generator().manual_seed(d))
    what = f"GINE hub gx d={d} F={F}"
    seen = []
    o32 = _aggregate_grads(x, ei, ea, W, b, gz, torch.float32)
    o64 = _aggregate_grads(x, ei, ea, W, b, gz, torch.float64, seen=seen)
    _check_gates({"message pre-activation": seen}, {"message pre-activation": _pre_bound(x, ei, ea, W, b)}, what)
    # the toothed variant: without the edge leaving the hub whose cotangent row is largest
    from_hub = torch.nonzero(ei[0] == 1).flatten()
    skip = int(from_hub[gz[ei[1][from_hub]].abs().max(1).values.argmax()])
    d64 = _aggregate_grads(x, ei, ea, W, b, gz, torch.float64, skip=skip)
    leaves = [t.detach().to(DEV).requires_grad_(True) for t in (x, W, b)]
    rel = Relation(ei.to(DEV), HUB_N, HUB_N, both=True)
    z = Fh.GINEAggregateFn.apply(leaves[0], ea.to(DEV), leaves[1], leaves[2], rel, 0.0)
    z.backward(gz.to(DEV))
    got = dict(zip(("x.x", "x.W", "x.b"), (t.grad for t in leaves)))
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    assert "x.x" in reached
    teeth(got, o32, o64, reached, what)


# --------------------------------------------------------------------------- #
# 4. flag word
# --------------------------------------------------------------------------- #
def test_short_edge_attr_is_refused_and_a_bad_node_id_is_flagged_and_skipped():
    N, E, F, De = 40, 90, 16, 3
    ref, prod, ei, x, ea, gy = _layer_case(N, E, F, F, De, 7)
    with pytest.raises(ValueError, match="edges"):
        prod(x.to(DEV), ei.to(DEV), ea[:-1].to(DEV))
    # one edge names node N: hscn_csr_build leaves it out of both CSRs and raises the flag; the walks read rowptr
    # ranges only (which hold valid entries only) and the per-edge kernel tests both ids before it reads a row, so the
    # operator computes the graph without that edge
    bad = ei.clone()
    bad[0, 11] = N
    keep = torch.ones(E, dtype=torch.bool)
    keep[11] = False
    rel = Relation(bad.to(DEV), N, N, both=True)
    assert int(rel.csr.flag.item()) != 0
    xd = x.to(DEV).requires_grad_(True)
    out = prod(xd, rel, ea.to(DEV))
    out.backward(gy.to(DEV))
    with pytest.raises(IndexError):
        rel.check()
    o32, out32 = _ref_step(ref, x, bad[:, keep], ea[keep], gy, torch.float32)
    o64, out64 = _ref_step(ref, x, bad[:, keep], ea[keep], gy, torch.float64)
    referee_all({"out": out}, {"out": out32}, {"out": out64}, "GINE with a skipped edge")
    referee_all(grads_of(prod, x=xd), o32, o64, "GINE with a skipped edge")


# --------------------------------------------------------------------------- #
# 5. capture
# --------------------------------------------------------------------------- #
def test_forward_and_backward_replay_from_a_captured_graph():
    """Forward and backward over a prebuilt Relation recorded with torch.cuda.graph replay bit-identically to the
    eager calls, for new values of x: no launch depends on a host read."""
    N, E, F, H, De = 64, 400, 16, 16, 3
    ref, prod, ei, x0, ea, gy = _layer_case(N, E, F, H, De, 11)
    rel = Relation(ei.to(DEV), N, N, both=True)
    x = x0.to(DEV).requires_grad_(True)
    ead, gyd = ea.to(DEV), gy.to(DEV)
    leaves = [x] + [p for _, p in prod.named_parameters()]
    names = ["out", "g_x"] + ["g_" + n for n, _ in prod.named_parameters()]
    values = [torch.randn(N, F, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (1, 2)]

    def run():
        y = prod(x, rel, ead, act="relu")
        return [y] + list(torch.autograd.grad(y, leaves, gyd))

    eager = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for v in values + values:
            with torch.no_grad():
                x.copy_(v)
            eager.append([t.clone() for t in run()])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for v, want in zip(values, eager[2:]):
        with torch.no_grad():
            x.copy_(v)
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(names, outs, want):
            assert torch.equal(a, b), name
    assert not torch.equal(eager[2][0], eager[3][0])


# --------------------------------------------------------------------------- #
# 6. models
# --------------------------------------------------------------------------- #
def _model_pair(F, H, C, De, task_level, batch, seed):
    from graph_hscn.train import batching
    torch.manual_seed(seed)
    ref = GO.GINEModelRef(F, H, C, 3, De, task_level)
    pm = MPNN(CONV_DICT["gine"], ACT_DICT["relu"], F, H, C, 3, dropout=0.0, task_level=task_level).to(DEV)
    bd = batching.to_device(pm, batch, DEV)
    with torch.no_grad():
        pm._forward(bd)                                    # edge_dim = -1: lin is sized by its first call
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    return ref, pm, bd


MODEL_SEED = 93     # chosen on the CPU so that the gate condition holds (module docstring); asserted in the test


def test_gine_mpnn_on_peptides_under_the_float64_referee():
    from graph_hscn.train.train import eval_epoch, train_epoch
    graphs = make_dataset("peptides_func", 8, seed=MODEL_SEED, edge_features=True)
    b = Batch.from_data_list(graphs)
    assert b.edge_attr.dtype == torch.int64 and b.edge_attr.shape == (b.edge_index.size(1), 3)
    ref, pm, bd = _model_pair(9, 16, 10, 3, "graph", b, MODEL_SEED)
    assert bd.edge_attr.dtype == torch.float32
    B = 8
    g = torch.randn(B, 10, generator=torch.Generator().manual_seed(1))

    def run(dtype, skip=None):
        m = copy.deepcopy(ref).to(dtype)
        seen = {}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        out = m(b.x.to(dtype), b.edge_index, b.edge_attr.to(dtype), b.batch, B, skip)
        out.backward(g.to(dtype))
        return {"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()}, out.detach(), seen

    o32, out32, gates32 = run(torch.float32)
    o64, out64, gates64 = run(torch.float64)
    assert len(gates64) == 3 * 2 + 2
    for tag, v64 in gates64.items():
        bound = 2.0 * float((gates32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"GINE MPNN {tag}")
    c0 = ref.conv_layers[0]
    skip = _largest_message(b.x.float(), b.edge_index, b.edge_attr.float(), c0.lin.weight.detach(), c0.lin.bias.detach())
    d64, dout64, _ = run(torch.float64, skip=skip)

    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == (B, 10)
    pred.backward(g.to(DEV))
    what = "GINE MPNN peptides B=8"
    referee_all({"pred": pred}, {"pred": out32}, {"pred": out64}, what)
    teeth({"pred": pred}, {"pred": out32}, {"pred": out64}, {"pred": dout64}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values()) and len(got) == 3 * 6
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    # every tensor sees the removed edge, but for the last layer's two MLP biases: behind the mean pool the last bias
    # has the gradient mean(g) whatever the graph, and nn.0.bias the gated column sums of g W2, which change only if a
    # hidden gate of that layer flips
    assert set(o64) - set(reached) <= {"p.conv_layers.2.nn.0.bias", "p.conv_layers.2.nn.2.bias"}, sorted(reached)
    teeth(got, o32, o64, reached, what)

    # one Adam iteration through the training loop lowers the loss on the same batch
    opt = torch.optim.Adam(pm.parameters(), lr=1e-3)
    before = train_epoch(0, None, [b], pm, opt, "cross_entropy", None, 1, False)[0]
    after = eval_epoch(1, None, [b], pm, "cross_entropy", None, "Test")[0]
    assert np.isfinite(before) and after < before, (before, after)


def test_gine_mpnn_node_and_link_levels():
    from graph_hscn import metrics
    from graph_hscn.loss import criterion
    from graph_hscn.train import batching
    from graph_hscn.train.train import eval_epoch
    # node level: PascalVOC-SP-shaped graphs, float edge features, one class index per node
    graphs = make_dataset("pascalvoc_sp_node", 2, seed=0, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(0)
    node = MPNN(CONV_DICT["gine"], ACT_DICT["relu"], 14, 16, 21, 3, dropout=0.0, task_level="node").to(DEV)
    bd = batching.to_device(node, b, DEV)
    pred, y = batching.forward(node, bd)
    assert pred.shape == (b.num_nodes, 21) and y.shape == (b.num_nodes,)
    loss, _ = criterion("weighted_cross_entropy", pred, y)
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in node.parameters())
    l, perf = eval_epoch(0, None, DataLoader(graphs, 2), node, "weighted_cross_entropy", metrics.eval_hip("f1_macro"), "Test")
    assert np.isfinite(l) and 0.0 <= perf <= 1.0
    # link level: PCQM-Contact-shaped graphs, integer bond features, one score per candidate pair
    graphs = make_dataset("pcqm_contact_link", 4, seed=0, edge_features=True)
    b = Batch.from_data_list(graphs)
    link = MPNN(CONV_DICT["gine"], ACT_DICT["relu"], 9, 16, 8, 3, dropout=0.0, task_level="link").to(DEV)
    bd = batching.to_device(link, b, DEV)
    scores, labels = batching.forward(link, bd)
    assert scores.shape == labels.shape == (b.edge_label_index.size(1),)
    loss, _ = criterion("cross_entropy", scores, labels)
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in link.parameters())
    l, mrr = eval_epoch(0, None, DataLoader(graphs, 4), link, "cross_entropy", None, "Test", link_metric="mrr")
    assert np.isfinite(l) and 0.0 < mrr <= 1.0


def test_resident_engines_refuse_gine_by_name_and_auto_runs_layered():
    from types import SimpleNamespace

    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    graphs = make_dataset("peptides_func", 4, seed=0, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(0)
    pm = MPNN(CONV_DICT["gine"], ACT_DICT["relu"], 9, 16, 10, 3, dropout=0.0).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(bd)
    assert pm.last_engine == "layered" and out.shape == (4, 10)
    pm.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="convolution GINE"):
        pm(bd)
    pm.engine = "layered"
    with pytest.raises(RuntimeError, match="convolution GINE"):
        MPNNResidentTrainStep(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="convolution GINE"):
        batching.resident_step(pm, bd, "cross_entropy")            # what replay.CapturedStep builds its step with
    with pytest.raises(RuntimeError, match="convolution GINE"):
        DeviceEvaluator(graphs, pm, "cross_entropy", 4).run()
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="convolution GINE"):
        fit_resident(None, opt, cfg, graphs, [], pm, 4)
