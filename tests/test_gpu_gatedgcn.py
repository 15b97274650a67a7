"""GatedGCN on the HIP path (csrc/gatedgcn.hip) against the plain-torch restatement of tests/gatedgcn_oracle.py.

Tolerances are the project's own (tests/helpers.py), no new constants:

  * the new edge features e^ by ``f64_close`` with n = 3 and mag = |Dx_i| + |Ex_j| + |Ce_k| (two additions);
  * the node output h by ``check_f64`` with the bound derived in ``_h_bound`` (below), and the same bound must REJECT the
    float64 value with the single edge removed that changes h most;
  * every gradient by ``referee_all`` (float32 and float64 restatements as the two oracles) with ``teeth``: the float64
    run with one edge removed must be rejected.

The bound of h, element by element, to first order in u = 2^-24 (``f64_close`` supplies the factor 3 for the second-order
terms and the output rounding); i the node, k its incoming edges, j = src_k, m_k = |Dx_i| + |Ex_j| + |Ce_k|:

  e^_k      two roundings, each of a partial sum no larger than m_k:      d e_k <= 3 u m_k            (the bar of e^ itself)
  s_k       sigmoid is Lipschitz with constant 1/4; the library call -- expf (1 ulp = 2u), the addition of 1 (u), the
            division (u), the sensitivity of 1 / (1 + t) to t being t / (1 + t) <= 1 -- adds 4u relative:
                                                                          d s_k <= 3/4 u m_k + 4 u s_k
  num_i     deg_i products s_k Bx_j (u each) summed in order (deg_i u on the sum of absolute terms):
            d num <= sum_k d s_k |Bx_j| + (deg_i + 1) u NUM <= 3/4 u sum_k m_k |Bx_j| + (deg_i + 5) u NUM,  NUM = sum_k s_k |Bx_j|
  den_i     d den <= sum_k d s_k + deg_i u den          <= 3/4 u sum_k m_k + (deg_i + 4) u den
  den + eps one rounding, and the float32 value of 1e-6:                  d (den + eps) <= d den + 2 u (den + eps)
  q_i       = num / (den + eps):      d q <= (d num + |q| d (den + eps)) / (den + eps) + u |q|
  h_i       = Ax_i + q_i:             d h <= d q + u (|Ax_i| + |q_i|)

Input condition, asserted on the float64 reference with no exclusion: every node with an incoming edge has
den >= 1e-3 in every channel (Dx, Ex, Ce are drawn with standard deviation 0.7, so |e^| stays below about 6 and every
gate above 2e-3).  The gate is smooth: the only kinks are the ReLUs after the layers, in the feed-forward blocks and in
the heads; their condition is the one tests/test_gpu_gine.py states for its model case (every ReLU input of the float64
run farther from zero than 4 x the referee's own limit for that tensor); seeds were chosen on the CPU so that it holds."""
import copy

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT, GPSConfig
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.model.mpnn import MPNN
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GatedGCNLayer
from graph_hscn.structure import Relation
from tests import gatedgcn_oracle as GG
from tests.helpers import (DEV, KinkGuard, TermMagnitudes, check_f64, f64_close, grads_of, most_changed, referee_all,
                           teeth)

pytestmark = pytest.mark.gpu

LONG, CHUNK = Fh.GATEDGCN_LONG_ROW, Fh.GATEDGCN_CHUNK
NAMES = ("Ax", "Bx", "Dx", "Ex", "Ce")


# --------------------------------------------------------------------------- #
# inputs, the bound, the two evaluations
# --------------------------------------------------------------------------- #
def _multigraph(N, E, seed):
    """The shape of tests/test_gpu_gine.py: [2, E] in RANDOM edge order (so that the CSR's eid[slot] != slot), the last
    four nodes isolated, nodes 1 and 2 with a self loop each, the first two random edges occurring three times."""
    g = torch.Generator().manual_seed(seed)
    live = max(N - 4, 1)
    base = torch.randint(0, live, (2, E - 6), generator=g)
    extra = torch.tensor([[1 % live, 2 % live], [1 % live, 2 % live]])
    ei = torch.cat([base, extra, base[:, :2], base[:, :2]], 1)
    return ei[:, torch.randperm(E, generator=g)].contiguous()


def _inputs(N, E, H, seed):
    """(Ax, Bx, Dx, Ex, Ce), float32; the three summands of e^ with standard deviation 0.7."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(N, H, generator=g), torch.randn(N, H, generator=g), 0.7 * torch.randn(N, H, generator=g),
            0.7 * torch.randn(N, H, generator=g), 0.7 * torch.randn(E, H, generator=g))


def _h_bound(t64, ei):
    """The bound of h in units of u = 2^-24 (module docstring), [N, H]; also (h64, e64, mags)."""
    Ax = t64[0]
    h64, e64 = GG.aggregate(*t64, ei)
    m = GG.magnitudes(*t64, ei)
    deg, den, eps = m["deg"], m["den"], GG.EPS
    q = (h64 - Ax).abs()
    d_num = 0.75 * m["dsumB"] + (deg + 5) * m["num"]
    d_den = 0.75 * m["dsum"] + (deg + 4) * den + 2 * (den + eps)
    bound = (d_num + q * d_den) / (den + eps) + q + Ax.abs() + q
    return bound, h64, e64, m


def _most_changing_edge(t64, ei):
    """The edge whose removal from num and den changes h most (max norm), found without E evaluations."""
    Ax, Bx = t64[0], t64[1]
    h64, e64 = GG.aggregate(*t64, ei)
    num, den = GG.sums(Bx, e64, ei)
    s = torch.sigmoid(e64)
    dst = ei[1]
    q_without = (num[dst] - s * Bx[ei[0]]) / (den[dst] - s + GG.EPS)
    return int((q_without - (h64 - Ax)[dst]).abs().max(1).values.argmax())


def _hip(t, ei, rel=None, needs=()):
    """The operator on the device: leaves (those named in ``needs`` require a gradient), h, e^, the relation."""
    N = t[0].size(0)
    rel = rel if rel is not None else Relation(ei.to(DEV), N, N)
    leaves = [x.detach().to(DEV).requires_grad_(n in needs) for n, x in zip(NAMES, t)]
    h, e = Fh.GatedGCNAggregateFn.apply(*leaves, rel)
    return leaves, h, e, rel


def _check_forward(t, ei, what, wrong_rows=False):
    _, h, e, rel = _hip(t, ei)
    t64 = [x.double() for x in t]
    bound, h64, e64, m = _h_bound(t64, ei)
    reached = m["deg"].flatten() > 0
    assert bool((m["den"][reached] >= 1e-3).all()), f"{what}: a gate sum below 1e-3"
    assert f64_close(e, e64, m["e"], 3, what=what + " e^"), what
    assert e.shape == (ei.size(1), t[0].size(1)) and h.shape == t[0].shape
    assert torch.equal(h.cpu()[~reached], t[0][~reached]), f"{what}: an isolated node's h is not Ax bit for bit"
    if ei.size(1) == 0:
        assert f64_close(h, h64, bound, 1, what=what + " h"), what
        return h, e
    dropped, _ = GG.aggregate(*t64, ei, skip=_most_changing_edge(t64, ei))
    check_f64(h, h64, bound, 1, dropped, what=what + " h")
    if wrong_rows:
        # the Ce row of a CSR slot is Ce[eid[slot]]: a kernel that takes Ce[slot] computes the graph with Ce permuted
        slot_edge = torch.argsort(ei[1], stable=True)
        assert not torch.equal(slot_edge, torch.arange(ei.size(1)))
        Ce_slot = torch.empty_like(t64[4])
        Ce_slot[slot_edge] = t64[4]
        h_slot, e_slot = GG.aggregate(*t64[:4], Ce_slot, ei)
        assert not f64_close(h, h_slot, bound, 1), f"{what}: the bound of h cannot tell Ce[eid[slot]] from Ce[slot]"
        assert not f64_close(e, e_slot, m["e"], 3), f"{what}: the bound of e^ cannot tell Ce[eid[slot]] from Ce[slot]"
        # ... and e^ is stored at row eid[slot]: rows written in slot order must fail
        assert not f64_close(e, e64[slot_edge], m["e"], 3), f"{what}: the bound of e^ cannot tell edge order from slot order"
    assert int(rel.csr.flag.item()) == 0
    return h, e


def _oracle_grads(t, ei, gh, ge, dtype, needs=NAMES, skip=None):
    leaves = [x.detach().clone().to(dtype).requires_grad_(n in needs) for n, x in zip(NAMES, t)]
    h, e = GG.aggregate(*leaves, ei, skip)
    loss = (h * gh.to(dtype)).sum()
    if ge is not None:
        loss = loss + (e * ge.to(dtype)).sum()
    loss.backward()
    return {"x." + n: (None if x.grad is None else x.grad.detach().clone()) for n, x in zip(NAMES, leaves)}


def _hip_grads(t, ei, gh, ge, needs=NAMES, rel=None):
    N = t[0].size(0)
    rel = rel if rel is not None else Relation(ei.to(DEV), N, N, both=True)
    leaves, h, e, _ = _hip(t, ei, rel, needs)
    loss = (h * gh.to(DEV)).sum()
    if ge is not None:
        loss = loss + (e * ge.to(DEV)).sum()
    loss.backward()
    return {"x." + n: (None if x.grad is None else x.grad.detach().clone()) for n, x in zip(NAMES, leaves)}, h, e


def _cotangents(N, E, H, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(N, H, generator=g), torch.randn(E, H, generator=g)


def _drop_candidates(t, ei):
    """Edges to remove for the teeth: the one that changes h most and the ones with the largest rows of Bx and Ce."""
    t64 = [x.double() for x in t]
    k = {_most_changing_edge(t64, ei), int(t64[4].abs().max(1).values.argmax()),
         int(t64[1][ei[0]].abs().max(1).values.argmax())}
    return sorted(k)


def _referee_grads(t, ei, gh, ge, what, needs=NAMES, expect=None):
    o32 = _oracle_grads(t, ei, gh, ge, torch.float32, needs)
    o64 = _oracle_grads(t, ei, gh, ge, torch.float64, needs)
    got, h, e = _hip_grads(t, ei, gh, ge, needs)
    referee_all(got, o32, o64, what)
    drops = [_oracle_grads(t, ei, gh, ge, torch.float64, needs, skip=k) for k in _drop_candidates(t, ei)]
    reached = most_changed(o64, drops)
    expect = {"x." + n for n in needs if n != "Ax"} if expect is None else expect      # d Ax = gh whatever the graph
    assert expect <= set(reached), (what, sorted(reached))
    teeth(got, o32, o64, reached, what)
    return got, h, e


# --------------------------------------------------------------------------- #
# 1. / 2. forward at every width; wrong rows must fail
# --------------------------------------------------------------------------- #
# H % 4 == 0: 16-byte lanes, otherwise scalar lanes; 68: 17 lanes per row, idle lanes at the end of the block; 33 / 17
# / 3: scalar lane groups of odd width; 260: 65 float4 lanes' worth, a second column pass (VEC = 4); 70: a second
# column pass on the scalar path (more than 64 columns, added to the issue's list); 512: the envelope's edge.
WIDTHS = [1, 3, 4, 16, 17, 33, 64, 68, 70, 260, 512]


@pytest.mark.parametrize("H", WIDTHS)
def test_forward_matches_float64_at_every_width(H):
    N, E = 40, 160
    ei = _multigraph(N, E, seed=H)
    deg = torch.bincount(ei[1], minlength=N)
    assert int((deg == 0).sum()) >= 4 and bool((ei[0] == ei[1]).any())
    assert torch.unique(ei[0] * N + ei[1]).numel() < E                     # repeated edges
    _check_forward(_inputs(N, E, H, seed=H), ei, f"GatedGCN forward H={H}", wrong_rows=True)


# --------------------------------------------------------------------------- #
# 3. structure edges
# --------------------------------------------------------------------------- #
def test_no_edges_gives_ax_and_exact_zero_gradients():
    N, H = 7, 9
    t = _inputs(N, 0, H, seed=1)
    ei = torch.zeros(2, 0, dtype=torch.int64)
    h, e = _check_forward(t, ei, "GatedGCN E=0")
    assert torch.equal(h.cpu(), t[0]) and e.shape == (0, H)
    gh, ge = _cotangents(N, 0, H, 1)
    got, _, _ = _hip_grads(t, ei, gh, ge, rel=Relation(ei.to(DEV), N, N))
    assert torch.equal(got["x.Ax"].cpu(), gh)
    for n in ("Bx", "Dx", "Ex"):
        assert got["x." + n] is not None and got["x." + n].shape == (N, H) and not bool(got["x." + n].any()), n
    assert got["x.Ce"] is not None and got["x.Ce"].shape == (0, H)


def test_one_node_with_one_self_loop():
    t = _inputs(1, 1, 16, seed=2)
    ei = torch.zeros(2, 1, dtype=torch.int64)
    _check_forward(t, ei, "GatedGCN N=1, one loop")
    gh, ge = _cotangents(1, 1, 16, 2)
    _referee_grads(t, ei, gh, ge, "GatedGCN N=1, one loop")


def _hub_graph(N, d, seed):
    """Node 0 receives ``d`` edges and node 1 sends ``d`` (repeated edges from / to the other nodes), plus 2 N random
    edges; random edge order (tests/test_gpu_gine.py)."""
    g = torch.Generator().manual_seed(seed)
    others = torch.arange(d) % (N - 2) + 2
    ei = torch.cat([torch.stack([others, torch.zeros(d, dtype=torch.int64)]),
                    torch.stack([torch.ones(d, dtype=torch.int64), others]),
                    torch.randint(2, N, (2, 2 * N), generator=g)], 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


HUB_N = 24


# H = 16: 4 lanes per row, 64 lane groups, every chunk of a split row in one round; H = 17: scalar lanes, 15 lane groups
# and one idle lane at the end of the block.  At the threshold, one above it, and one above a chunk boundary of a split
# row: in-degree of node 0 (the forward and the backward's target walk), out-degree of node 1 (the source walk).
@pytest.mark.parametrize("H", [16, 17])
@pytest.mark.parametrize("d", [LONG, LONG + 1, LONG + CHUNK + 1])
def test_hub_rows_forward_and_backward(H, d):
    ei = _hub_graph(HUB_N, d, seed=d)
    indeg, outdeg = torch.bincount(ei[1], minlength=HUB_N), torch.bincount(ei[0], minlength=HUB_N)
    assert int(indeg[0]) == d and int(outdeg[1]) == d
    assert int(indeg[1:].max()) < LONG and int(outdeg[0]) < LONG and int(outdeg[2:].max()) < LONG
    E = ei.size(1)
    t = _inputs(HUB_N, E, H, seed=H + d)
    what = f"GatedGCN hub d={d} H={H}"
    _check_forward(t, ei, what, wrong_rows=True)
    gh, ge = _cotangents(HUB_N, E, H, d)
    _referee_grads(t, ei, gh, ge, what)


def _peptides_batch(graphs, H, seed):
    b = Batch.from_data_list(graphs)
    return b, _inputs(b.num_nodes, b.edge_index.size(1), H, seed)


def test_a_batch_of_three_peptides_graphs():
    graphs = make_dataset("peptides_func", 3, seed=0, edge_features=True)
    b, t = _peptides_batch(graphs, 16, seed=3)
    what = "GatedGCN 3 peptides graphs"
    _check_forward(t, b.edge_index, what)
    gh, ge = _cotangents(b.num_nodes, b.edge_index.size(1), 16, 3)
    _referee_grads(t, b.edge_index, gh, ge, what)


# --------------------------------------------------------------------------- #
# 4. an edge the CSR build leaves out
# --------------------------------------------------------------------------- #
def test_a_flagged_edge_takes_no_part_and_its_rows_are_zero():
    N, E, H = 40, 160, 16
    ei = _multigraph(N, E, seed=7)
    t = _inputs(N, E, H, seed=7)
    gh, ge = _cotangents(N, E, H, 7)
    bad = ei.clone()
    bad[0, 11] = N                                  # hscn_csr_build leaves the edge out of both CSRs and raises the flag
    keep = torch.ones(E, dtype=torch.bool)
    keep[11] = False
    rel = Relation(bad.to(DEV), N, N, both=True)
    assert int(rel.csr.flag.item()) != 0
    got, h, e = _hip_grads(t, bad, gh, ge, rel=rel)
    with pytest.raises(IndexError):
        rel.check()
    t_keep = t[:4] + (t[4][keep],)
    want, h_keep, e_keep = _hip_grads(t_keep, bad[:, keep], gh, ge[keep])
    assert torch.equal(h, h_keep)
    assert not bool(e[11].any()) and torch.equal(e[keep.to(DEV)], e_keep)
    assert not bool(got["x.Ce"][11].any()) and torch.equal(got["x.Ce"][keep.to(DEV)], want["x.Ce"])
    for n in ("Ax", "Bx", "Dx", "Ex"):
        assert torch.equal(got["x." + n], want["x." + n]), n
    # the same with the e^ cotangent absent (the sweep of ge is the backward's own)
    got, _, _ = _hip_grads(t, bad, gh, None, rel=rel)
    want, _, _ = _hip_grads(t_keep, bad[:, keep], gh, None)
    assert not bool(got["x.Ce"][11].any()) and torch.equal(got["x.Ce"][keep.to(DEV)], want["x.Ce"])


# --------------------------------------------------------------------------- #
# 5. gradients
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("H", [3, 16, 68])
def test_gradients_of_all_five_inputs(H):
    N, E = 40, 160
    ei = _multigraph(N, E, seed=H + 1)
    t = _inputs(N, E, H, seed=H + 1)
    gh, ge = _cotangents(N, E, H, H)
    what = f"GatedGCN gradients H={H}"
    got, _, _ = _referee_grads(t, ei, gh, ge, what)
    assert torch.equal(got["x.Ax"].cpu(), gh)
    # the e^ cotangent absent: the last layer of a stack drops its edge output
    got, _, _ = _referee_grads(t, ei, gh, None, what + ", no e^ cotangent")
    assert all(v is not None for v in got.values())
    # only Bx asks: None where the oracle has None
    got, _, _ = _referee_grads(t, ei, gh, ge, what + ", Bx alone", needs=("Bx",))
    assert got["x.Bx"] is not None and all(got["x." + n] is None for n in NAMES if n != "Bx")
    # only Ce asks (a first layer behind a trainable edge encoder): the target-keyed pass alone
    got, _, _ = _referee_grads(t, ei, gh, ge, what + ", Ce alone", needs=("Ce",))
    assert got["x.Ce"] is not None and all(got["x." + n] is None for n in NAMES if n != "Ce")


def test_only_the_edge_output_is_used():
    """A loss on e^ alone: autograd hands the operator no cotangent for h."""
    N, E, H = 40, 160, 16
    ei = _multigraph(N, E, seed=21)
    t = _inputs(N, E, H, seed=21)
    _, ge = _cotangents(N, E, H, 21)
    leaves, h, e, _ = _hip(t, ei, Relation(ei.to(DEV), N, N, both=True), NAMES)
    (e * ge.to(DEV)).sum().backward()
    got = {"x." + n: x.grad for n, x in zip(NAMES, leaves)}
    zero = torch.zeros(N, H)
    o32 = _oracle_grads(t, ei, zero, ge, torch.float32)
    o64 = _oracle_grads(t, ei, zero, ge, torch.float64)
    referee_all(got, o32, o64, "GatedGCN, e^ cotangent alone")
    assert not bool(got["x.Ax"].any()) and not bool(got["x.Bx"].any())


# --------------------------------------------------------------------------- #
# 6. reproducibility
# --------------------------------------------------------------------------- #
def test_two_runs_and_two_batch_positions_give_the_same_bits():
    N, E, H = 40, 160, 16
    ei = _multigraph(N, E, seed=5)
    t = _inputs(N, E, H, seed=5)
    gh, ge = _cotangents(N, E, H, 5)
    a, ha, ea = _hip_grads(t, ei, gh, ge)
    b, hb, eb = _hip_grads(t, ei, gh, ge)
    assert torch.equal(ha, hb) and torch.equal(ea, eb)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # one graph first and last in a batch of three: its rows of h and e^ are the same bits
    graphs = make_dataset("peptides_func", 3, seed=1, edge_features=True)
    H = 16
    per_graph = [_inputs(g.num_nodes, g.edge_index.size(1), H, seed=10 + i) for i, g in enumerate(graphs)]

    def run(order):
        bt = Batch.from_data_list([graphs[i] for i in order])
        t = tuple(torch.cat([per_graph[i][c] for i in order]) for c in range(5))
        _, h, e, _ = _hip(t, bt.edge_index)
        return h.cpu(), e.cpu()

    h_first, e_first = run([0, 1, 2])
    h_last, e_last = run([1, 2, 0])
    n0, e0 = graphs[0].num_nodes, graphs[0].edge_index.size(1)
    assert torch.equal(h_first[:n0], h_last[-n0:]) and torch.equal(e_first[:e0], e_last[-e0:])
    assert not torch.equal(h_first[:n0], h_last[:n0])


# --------------------------------------------------------------------------- #
# 7. modules and models
# --------------------------------------------------------------------------- #
def _check_gates(g32, g64, what):
    """Every ReLU input of the float64 run farther from zero than 4 x the referee's own limit for its tensor."""
    assert set(g32) == set(g64) and g64
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"{what} {tag}")


def _row_dropped(o64, key, cot):
    """``o64`` with the largest row removed from the bias gradient ``key`` = sum_r cot[r]: the toothed reference of a
    sum that is zero in exact arithmetic whatever the graph (no removed edge reaches it)."""
    d = dict(o64)
    d[key] = o64[key] - cot[int(cot.abs().max(1).values.argmax())]
    return d


def _watch_cotangent(module, store, key):
    """The cotangent of ``module``'s output (its bias gradient's terms), kept under ``key``."""
    return module.register_forward_hook(
        lambda m, a, out: out.register_hook(lambda g: store.__setitem__(key, g.detach().double().clone())) and None)


LAYER_D, LAYER_SEED = 16, 0
# d A.bias = sum_i (cotangent of A x_i), in front of bn_node_x in training mode: the batch norm removes a column's
# shift, so the sum is zero in exact arithmetic and rounding residue in any float32 evaluation
_A_BIAS = "in front of a BatchNorm in training mode, which removes a column's shift: the cotangent columns sum to 0"
_NORM_WEIGHT = "in front of a BatchNorm, which removes a column's shift and scale: the cotangent columns sum to ~0"
_B_BIAS = ("a shift of every Bx row moves every non-isolated h row alike (up to eps / den), which bn_node_x removes: "
           "on graphs without isolated nodes the cotangent columns sum to ~0")


def _layer_run(ref, ei, x, ea, gx, ge, dtype, skip=None, masks=None, terms=False):
    m = copy.deepcopy(ref).to(dtype)
    m.train()
    seen, cot = {}, {}
    m.watch = lambda tag, t: seen.__setitem__(tag, t.detach().double())
    hook = _watch_cotangent(m.A, cot, "p.A.bias")
    # the chain behind a parameter: the five Linears and two BatchNorms are counted by TermMagnitudes; the gated sums
    # (largest in-degree terms each for num and den, the sigmoid, the quotient and the final addition: + 8) are added here
    tm = TermMagnitudes(m, chain_extra=int(torch.bincount(ei[1]).max()) + 8) if terms else None
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    ee = ea.detach().clone().to(dtype).requires_grad_(True)
    h, e = m(xx, ei, ee, skip, None if masks is None else tuple(k.to(dtype) for k in masks))
    ((h * gx.to(dtype)).sum() + (e * ge.to(dtype)).sum()).backward()
    hook.remove()
    if tm is not None:
        tm.close()
    g = {"x.x": xx.grad.detach().clone(), "x.edge_attr": ee.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    out = {"x": h.detach(), "e": e.detach()}
    out.update({"s." + n: b.detach().clone() for n, b in m.named_buffers() if "running" in n})
    return g, out, seen, cot, tm


def _layer_case(seed, N=40, E=160):
    torch.manual_seed(seed)
    ref = GG.GatedGCNLayerRef(LAYER_D, residual=True, norm="batch")
    g = torch.Generator().manual_seed(4000 + seed)
    ei = _multigraph(N, E, seed)
    return ref, ei, (torch.randn(N, LAYER_D, generator=g), torch.randn(E, LAYER_D, generator=g),
                     torch.randn(N, LAYER_D, generator=g), torch.randn(E, LAYER_D, generator=g))


def _layer_product(ref, dropout=0.0):
    prod = GatedGCNLayer(LAYER_D, dropout=dropout, residual=True, norm="batch", act="relu", edge_dim=LAYER_D).to(DEV)
    prod.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    return prod.train()


def _layer_step(prod, ei, x, ea, gx, ge):
    xd, ed = x.to(DEV).requires_grad_(True), ea.to(DEV).requires_grad_(True)
    h, e = prod(xd, ei.to(DEV), ed)
    ((h * gx.to(DEV)).sum() + (e * ge.to(DEV)).sum()).backward()
    out = {"x": h.detach(), "e": e.detach()}
    out.update({"s." + n: b.detach().clone() for n, b in prod.named_buffers() if "running" in n})
    return grads_of(prod, x=xd, edge_attr=ed), out


def test_gated_layer_in_training_mode_under_the_float64_referee():
    what = "GatedGCNLayer D=16 batch norm, residual"
    ref, ei, io = _layer_case(LAYER_SEED)
    o32, y32, g32, _, _ = _layer_run(ref, ei, *io, torch.float32)
    o64, y64, g64, cot, terms = _layer_run(ref, ei, *io, torch.float64, terms=True)
    assert set(g64) == {"node ReLU input", "edge ReLU input"}
    _check_gates(g32, g64, what)
    r64 = copy.deepcopy(ref).double()
    t64 = [lin(io[0].double()).detach() for lin in (r64.A, r64.B, r64.D, r64.E)] + [r64.C(io[1].double()).detach()]
    skip = _most_changing_edge(t64, ei)
    d64, dy64, _, _, _ = _layer_run(ref, ei, *io, torch.float64, skip=skip)
    prod = _layer_product(ref)
    got, y = _layer_step(prod, ei, *io)
    assert set(y) == {"x", "e", "s.bn_node_x.running_mean", "s.bn_node_x.running_var", "s.bn_edge_e.running_mean",
                      "s.bn_edge_e.running_var"}
    referee_all(y, y32, y64, what)                          # the two outputs and the four running statistics
    # (a removed edge keeps its row of e^: the edge output and its statistics are the forward test's to bite on)
    teeth(y, y32, y64, {k: dy64[k] for k in ("x", "s.bn_node_x.running_mean", "s.bn_node_x.running_var")}, what)
    assert all(v is not None for v in got.values()) and len(got) == 2 + 10 + 4
    referee_all(got, o32, o64, what, terms=terms, cancelling={"p.A.bias": _A_BIAS})
    terms.bound_teeth(got, o32, o64, [_row_dropped(o64, "p.A.bias", cot["p.A.bias"])], ["p.A.bias"], what)
    reached = most_changed(o64, [d64])
    # bn_edge_e's own gradients are sums over e^ rows and their fixed cotangents, which a removed edge leaves alone
    # (A.bias, zero in exact arithmetic, has had its teeth above: what a removed edge changes of it is float64 noise)
    reached.pop("p.A.bias", None)
    assert set(o64) - set(reached) == {"p.A.bias", "p.bn_edge_e.weight", "p.bn_edge_e.bias"}, sorted(reached)
    teeth(got, o32, o64, reached, what)


def test_gated_layer_dropout_masks_are_the_pinned_draws_and_differ():
    what = "GatedGCNLayer dropout 0.5"
    ref, ei, io = _layer_case(LAYER_SEED + 1)
    N, E = io[0].size(0), io[1].size(0)
    seed = 1234
    ones = torch.ones(max(N, E), LAYER_D, device=DEV)
    mask_x = Fh.dropout(ones[:N], p=0.5, training=True, seed=seed).cpu()
    mask_e = Fh.dropout(ones[:E], p=0.5, training=True, seed=seed + GatedGCNLayer.EDGE_SEED_OFFSET).cpu()
    assert set(mask_x.unique().tolist()) == {0.0, 2.0} and set(mask_e.unique().tolist()) == {0.0, 2.0}
    assert not torch.equal(mask_x, mask_e[:N])              # not the same draw
    assert not torch.equal(mask_e[:N], Fh.dropout(ones[:E], p=0.5, training=True, seed=seed).cpu()[:N])
    o32, y32, _, _, _ = _layer_run(ref, ei, *io, torch.float32, masks=(mask_x, mask_e))
    o64, y64, _, _, _ = _layer_run(ref, ei, *io, torch.float64, masks=(mask_x, mask_e))
    prod = _layer_product(ref, dropout=0.5)
    prod.dropout_seed = seed
    got, y = _layer_step(prod, ei, *io)
    referee_all(y, y32, y64, what)
    # without the masks the restatement is elsewhere: the bar sees a wrong mask
    _, plain64, _, _, _ = _layer_run(ref, ei, *io, torch.float64)
    teeth(y, y32, y64, {"x": plain64["x"], "e": plain64["e"]}, what)
    # every seed a GPS model hands to a node mask (dropout_seed + 4 i + k) is far from every edge mask's seed
    L = 16
    node_seeds = {seed + 4 * i + k for i in range(L) for k in range(4)}
    edge_seeds = {seed + 4 * i + GatedGCNLayer.EDGE_SEED_OFFSET for i in range(L)}
    assert not node_seeds & edge_seeds


# ---- the MPNN baseline --------------------------------------------------------------------------------------------
MODEL_SEEDS = {"graph": 2, "node": 22, "link": 0}      # chosen on the CPU so that the gate condition holds
MODEL_DATA = {"graph": ("peptides_func", 3, 9, 10), "node": ("pascalvoc_sp_node", 1, 14, 21),
              "link": ("pcqm_contact_link", 3, 9, 8)}


def _mpnn_reference(level):
    """Everything of a model case that is computed on the CPU (the seed search runs this alone)."""
    name, count, F, C = MODEL_DATA[level]
    seed = MODEL_SEEDS[level]
    graphs = make_dataset(name, count, seed=seed, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(seed)
    ref = GG.GatedGCNModelRef(F, 16, C, 3, int(b.edge_attr.size(1)), level)
    rows = {"graph": (int(b.num_graphs), C), "node": (int(b.num_nodes), C)}.get(level) or (int(b.edge_label_index.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))
    pairs = b.edge_label_index if level == "link" else None

    def run(dtype, skip=None):
        m = copy.deepcopy(ref).to(dtype)
        seen = {}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        out = m(b.x.to(dtype), b.edge_index, b.edge_attr.to(dtype), b.batch, int(b.num_graphs), pairs, skip)
        out.backward(gy.to(dtype))
        return {"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()}, out.detach(), seen

    c0 = copy.deepcopy(ref.conv_layers[0]).double()
    x64, e64 = b.x.double(), b.edge_attr.double()
    t64 = [lin(x64).detach() for lin in (c0.A, c0.B, c0.D, c0.E)] + [c0.C(e64).detach()]
    return ref, b, gy, run(torch.float32), run(torch.float64), run(torch.float64, _most_changing_edge(t64, b.edge_index))


def _mpnn_product(ref, b, F, C, level):
    from graph_hscn.train import batching
    pm = MPNN(CONV_DICT["gatedgcn"], ACT_DICT["relu"], F, 16, C, 3, dropout=0.0, task_level=level).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    with torch.no_grad():
        pm._forward(bd)                                    # edge_dim = -1: every C is sized by its first call
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    return pm, bd


@pytest.mark.parametrize("level", ["graph", "node", "link"])
def test_gatedgcn_mpnn_under_the_float64_referee(level):
    """The prediction bar is the reference's own error, 2 max|f32 - f64| + 8 2^-23 max|f64| (``referee``), as for the
    GINE model; graph level with the teeth on every tensor, node and link level with the forward and one backward."""
    what = f"GatedGCN MPNN {level} level"
    F, C = MODEL_DATA[level][2:]
    ref, b, gy, (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = _mpnn_reference(level)
    assert len(g64) == 2 * 2                               # node and edge output of the two hidden layers
    _check_gates(g32, g64, what)
    pm, bd = _mpnn_product(ref, b, F, C, level)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dy64}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values()) and len(got) == 3 * 10
    referee_all(got, o32, o64, what)
    if level == "graph":
        reached = most_changed(o64, [d64])
        # behind the mean pool the last layer's A.bias has the gradient mean(g) whatever the graph
        assert set(o64) - set(reached) <= {"p.conv_layers.2.A.bias"}, sorted(set(o64) - set(reached))
        teeth(got, o32, o64, reached, what)


def test_resident_entry_points_refuse_the_model_by_name_on_the_device():
    from types import SimpleNamespace

    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    graphs = make_dataset("peptides_func", 4, seed=0, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(0)
    pm = MPNN(CONV_DICT["gatedgcn"], ACT_DICT["relu"], 9, 16, 10, 3, dropout=0.0).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(bd)
    assert pm.last_engine == "layered" and out.shape == (4, 10)
    pm.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        pm(bd)
    pm.engine = "layered"
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        MPNNResidentTrainStep(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        batching.resident_step(pm, bd, "cross_entropy")            # what replay.CapturedStep builds its step with
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        DeviceEvaluator(graphs, pm, "cross_entropy", 4).run()
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        fit_resident(None, opt, cfg, graphs, [], pm, 4)


# ---- GPS with the gated local branch ------------------------------------------------------------------------------
GPS_D, GPS_HEADS, GPS_L = 16, 4, 2
# A second condition on the float64 REFERENCE, asserted with no exclusion: every column entering a gated layer's batch
# norm has |mean| <= 8 std.  A batch norm carries the rounding of its input into the normalised value amplified by
# (|x| + |mean|) / std (helpers.f64_close, "normalisation"), with a constant that depends on how an evaluation forms
# its sums, so two correct float32 evaluations drift apart by that factor.  The referee takes the float32 oracle's own
# distance as the yardstick and grants 8 ulp of the tensor's scale beyond it; an amplification within 8 keeps that part
# inside what the referee grants.  (In a stack the second layer's inputs come out of a LayerNorm and a ReLU, and a column
# of A x + aggregate can sit 30 standard deviations from zero.)  The seed was chosen on the CPU, from the reference alone:
# of the seeds 0..39 whose float64 run keeps its gates 1.4 x the required distance or more (0, 9, 29, 30, 38: ratios
# 6.5, 3.8, 11, 31, 8.2), the one with the best-conditioned batch-norm inputs.
GPS_SEED = 9
BN_MEAN_OVER_STD = 8.0


def _gps_reference():
    from tests.test_gpu_attention import _Terms
    graphs = make_dataset("peptides_func", 3, seed=GPS_SEED, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(GPS_SEED)
    ref = GG.GatedGPSRef(9, GPS_D, 10, GPS_L, GPS_HEADS, edge_dim=int(b.edge_attr.size(1)))
    gy = torch.randn(int(b.num_graphs), 10, generator=torch.Generator().manual_seed(1))
    bias_keys = {f"p.layers.{i}.conv.{n}.bias": (i, n) for i in range(GPS_L) for n in "AB"}

    def run(dtype, terms=False, **skips):
        m = copy.deepcopy(ref).to(dtype)
        m.train()                                          # the gated layers' batch norms in training mode
        seen, cot = {}, {"bn mean / std": 0.0}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        hooks = [_watch_cotangent(getattr(m.layers[i].conv, n), cot, k) for k, (i, n) in bias_keys.items()]
        for layer in m.layers:
            for bn in (layer.conv.bn_node_x, layer.conv.bn_edge_e):
                hooks.append(bn.register_forward_hook(lambda mod, a, out: cot.__setitem__(
                    "bn mean / std", max(cot["bn mean / std"],
                                         float((a[0].detach().mean(0).abs() / a[0].detach().std(0)).max())))))
        tm = None
        if terms:
            tm = _Terms(m)
            # what TermMagnitudes does not count itself: per gated layer the two sums over the largest in-degree, the
            # sigmoid, the quotient and the final addition (+ 8); the pool's segment
            tm.chain += GPS_L * (int(torch.bincount(b.edge_index[1]).max()) + 8) + int(torch.bincount(b.batch).max())
        out = m(b.x.to(dtype), b.edge_index, b.edge_attr.to(dtype), b.batch, b.ptr, int(b.num_graphs), None, **skips)
        out.backward(gy.to(dtype))
        for h in hooks:
            h.remove()
        if tm is not None:
            tm.close()
        g = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
        return g, out.detach(), seen, cot, tm

    return ref, b, gy, bias_keys, run


def test_gps_with_the_gated_local_branch_under_the_float64_referee():
    from graph_hscn.train import batching
    what = "GPS local_conv=gatedgcn, graph level"
    ref, b, gy, bias_keys, run = _gps_reference()
    o32, y32, g32, _, _ = run(torch.float32)
    o64, y64, g64, cot, terms = run(torch.float64, terms=True)
    assert len(g64) == GPS_L * 3 + 1           # per layer the two ReLU inputs of the gated layer and the feed-forward's
    _check_gates(g32, g64, what)
    print(f"   {what}: largest |mean| / std of a batch-norm input column = {cot['bn mean / std']:.2f}")
    assert cot["bn mean / std"] <= BN_MEAN_OVER_STD
    edge_drop = run(torch.float64, skip=int(b.edge_index.size(1)) // 2)
    drops = [edge_drop[0], run(torch.float64, att_skip=(0, 0))[0], run(torch.float64, pool_skip=0)[0]]
    drops += [_row_dropped(o64, k, cot[k]) for k in bias_keys]
    pm = GPS(9, GPS_D, 10, GPS_L, num_heads=GPS_HEADS, local_conv="gatedgcn", activation=ACT_DICT["relu"], dropout=0.0,
             norm="layer").to(DEV).train()
    bd = batching.to_device(pm, b, DEV)
    pm.edge_encoder.materialize(int(b.edge_attr.size(1)), bd.x)
    for layer in pm.layers:
        layer.conv.C.materialize(GPS_D, bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": edge_drop[1]}, what)
    got = grads_of(pm)
    # the last layer's edge output is dropped: its bn_edge_e sees no cotangent, on either side
    none = {f"p.layers.{GPS_L - 1}.conv.bn_edge_e.{n}" for n in ("weight", "bias")}
    assert {k for k, v in o64.items() if v is None} == none
    cancelling = {f"p.layers.{i}.attn.in_proj_bias": "the K third is zero in exact arithmetic (tests/test_gpu_attention.py)"
                  for i in range(GPS_L)}
    cancelling[f"p.layers.{GPS_L - 1}.norm2.bias"] = "equal parts of differing sign behind the mean pool (test_gpu_attention.py)"
    cancelling.update({k: (_A_BIAS if n == "A" else _B_BIAS) for k, (_, n) in bias_keys.items()})
    # A.weight / B.weight = (cotangent of A x / B x)^T x: bn_node_x removes a column's shift and scale, so the cotangent
    # columns sum to ~0 and are orthogonal to the normalised column (tests/test_gpu_layered_f64.py names a convolution's
    # weight in front of a BatchNorm for the same reason); a removed edge reaches them, so they have their teeth
    cancelling.update({f"p.layers.{i}.conv.{n}.weight": _NORM_WEIGHT for i in range(GPS_L) for n in "AB"})
    referee_all(got, o32, o64, what, terms=terms, cancelling=list(cancelling))
    terms.bound_teeth(got, o32, o64, drops, list(cancelling), what)
    reached = most_changed(o64, [edge_drop[0]])
    # edge_encoder: the tensor whose gradient exists only because edge_attr carries one
    assert {"p.edge_encoder.weight", "p.edge_encoder.bias", "p.node_encoder.weight", "p.layers.0.conv.C.weight",
            "p.layers.1.conv.E.weight", "p.lin_2.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, {k: v for k, v in reached.items() if k not in cancelling}, what)
    pm.check_flags()


def test_one_epoch_of_gps_with_gatedgcn_through_the_training_loop():
    from graph_hscn.train import batching
    from graph_hscn.train.train import eval_epoch, train_epoch
    graphs = make_dataset("peptides_func", 16, seed=2, edge_features=True)
    torch.manual_seed(2)
    pm = build_gps(GPSConfig("relu", local_conv_type="gatedgcn", hidden_channels=16, num_layers=2, num_heads=4,
                             dropout=0.1), 9, 10).to(DEV)
    loader = [Batch.from_data_list(graphs[:8]), Batch.from_data_list(graphs[8:])]
    with torch.no_grad():
        pm(batching.to_device(pm, loader[0], DEV))         # sizes edge_encoder and every C before the optimizer sees them
    opt = torch.optim.Adam(pm.parameters(), lr=1e-3)
    loss = train_epoch(0, None, loader, pm, opt, "cross_entropy", None, 1, False)[0]
    after = eval_epoch(1, None, loader, pm, "cross_entropy", None, "Test")[0]
    assert np.isfinite(loss) and np.isfinite(after)
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in pm.parameters())
