"""PNAConv on the HIP path (csrc/pna.hip) against the plain-torch restatement of tests/pna_oracle.py.

Every tensor -- the operator's output and its three gradients, the layer's and the models' predictions and parameter
gradients -- is held to ``helpers.referee`` with the restatement's float32 and float64 evaluations as the two oracles,
and ``helpers.teeth`` rejects the float64 run with one edge removed.  No new tolerance.

The operator's graph (``_graph``) is built, not drawn, so that every structure the kernels branch on is there at every
width, and so that min / max select the same edge in HIP, float32 and float64:

  * node Z has no in-edge, node O exactly one, node R two bit-identical ones (same source, same ``t`` row): R's variance
    is exactly 0 in both precisions and its min and max tie;
  * node G has exactly 256 in-edges (the last serial row), node H 257 (split into chunks of 64, the last chunk holding
    one slot; at F = 260 the workgroup has 4 lane groups for H's 5 chunks: a second round).  In H's row the source of
    slots 63 and 64 is HI -- above every other row of ``b`` in every column, with one ``t`` row for both: the argmax is
    in the first chunk and ties bit for bit across the chunk boundary -- and the source of slot 256 is LO, below every
    other: the argmin is in the last chunk;
  * node S sends 257 edges (the source walk's split row, a second round at F = 260);
  * apart from the two designated repeats no (source, target) pair occurs twice, and column f of ``b`` holds a
    permutation of a grid of spacing DELTA over the nodes (jitter DELTA / 8), ``t`` lies within DELTA / 4: two messages
    of a row differ by at least DELTA / 4 in every column, whatever the seed.

Preconditions, asserted on the float64 restatement and never on the code under test (``_preconditions``): the gap between
the best and the second-best message of every (node, column), min and max alike, is at least 1e-4 of the messages' max
magnitude apart from the designated ties, and every row of degree >= 2 without repeats has variance >= 1e-2.  The seeds
below were chosen on the CPU so that both hold."""
import copy

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT, MPNNConfig, PNAConfig
from graph_hscn.data import Batch, DataLoader
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import PNAConv
from graph_hscn.structure import Relation
from tests import gps_oracle as GPSO
from tests import pna_oracle as PO
from tests.helpers import DEV, grads_of, most_changed, referee_all, teeth

pytestmark = pytest.mark.gpu

LONG, CHUNK = Fh.PNA_LONG_ROW, Fh.PNA_CHUNK
DELTA = 1.0 / 64.0
ORD = 256                                     # ordinary nodes 0 .. 255: the sources of the long rows
HI, LO, H, G, Z, O, R, S = 256, 257, 258, 259, 260, 261, 262, 263
N_NODES = 264
WIDTHS = [1, 3, 4, 20, 260, 512]
ALL_AGGR, ALL_SCAL = PO.AGGREGATORS, PO.SCALERS
AVG_DEG_LOG = 1.25


# --------------------------------------------------------------------------- #
# the operator's graph and inputs
# --------------------------------------------------------------------------- #
def _graph(seed):
    """(edge_index [2, E], {name: edge numbers}) as the module docstring describes; the edge list is in random order
    (so that the CSR's eid[slot] != slot) except that H's in-edges keep their designated relative order."""
    g = torch.Generator().manual_seed(seed)
    edges = []
    src_h = torch.randperm(ORD, generator=g)[:254].tolist()
    row_h = src_h[:63] + [HI, HI] + src_h[63:] + [LO]                       # slots 0..256 of H
    assert len(row_h) == LONG + 1 and row_h[63] == row_h[64] == HI and row_h[256] == LO
    edges += [(s, H) for s in row_h]
    edges += [(s, G) for s in torch.randperm(ORD, generator=g).tolist()]   # exactly 256 distinct sources
    edges += [(S, d) for d in range(LONG + 1)]                              # S sends 257 edges: targets 0 .. 256
    for d in range(6):                                                      # a few ordinary rows of degree 9 .. 14
        edges += [(s, d) for s in (torch.randperm(ORD - 8, generator=g)[:8 + d] + 8).tolist()]
    edges += [(7, O), (9, R), (9, R), (Z, 3)]
    ei = torch.tensor(edges, dtype=torch.int64).t()
    E = ei.size(1)
    perm = torch.randperm(E, generator=g)
    ei = ei[:, perm]
    at_h = torch.nonzero(ei[1] == H).flatten()                              # H's edges back into their designated order
    ei[0, at_h] = torch.tensor(row_h)
    ei = ei.contiguous()
    at_r = torch.nonzero(ei[1] == R).flatten()
    names = {"h63": int(at_h[63]), "h64": int(at_h[64]), "h256": int(at_h[256]), "r0": int(at_r[0]), "r1": int(at_r[1]),
             "o": int(torch.nonzero(ei[1] == O).flatten()[0])}
    deg = torch.bincount(ei[1], minlength=N_NODES)
    assert int(deg[Z]) == 0 and int(deg[O]) == 1 and int(deg[R]) == 2 and int(deg[G]) == LONG and int(deg[H]) == LONG + 1
    assert int(torch.bincount(ei[0], minlength=N_NODES)[S]) == LONG + 1
    pairs = ei[0] * N_NODES + ei[1]
    assert torch.unique(pairs).numel() == E - 2                             # the two designated repeats, no other
    assert not torch.equal(torch.argsort(ei[1], stable=True), torch.arange(E))
    return ei, names


def _inputs(F, seed, with_t=True):
    ei, names = _graph(seed)
    g = torch.Generator().manual_seed(7000 + seed)
    E = ei.size(1)
    a = torch.rand(N_NODES, F, generator=g) * 2 - 1
    level = torch.stack([torch.randperm(N_NODES, generator=g) for _ in range(F)], 1).float() - (N_NODES - 1) / 2
    b = level * DELTA + (torch.rand(N_NODES, F, generator=g) - 0.5) * (DELTA / 4)
    b[HI] = (N_NODES / 2 + 4) * DELTA + torch.rand(F, generator=g) * DELTA
    b[LO] = -(N_NODES / 2 + 4) * DELTA - torch.rand(F, generator=g) * DELTA
    t = None
    if with_t:
        t = (torch.rand(E, F, generator=g) - 0.5) * (DELTA / 2)
        t[names["h64"]] = t[names["h63"]]
        t[names["r1"]] = t[names["r0"]]
    return ei, names, a, b, t, g


def _preconditions(a, b, t, ei, names, what):
    """On the float64 restatement: the gaps of min and max and the variances (module docstring)."""
    m = PO.messages(a.double(), b.double(), None if t is None else t.double(), ei)
    thr = 1e-4 * float(m.abs().max())
    dst = ei[1]
    deg = torch.bincount(dst, minlength=N_NODES)
    worst_gap, worst_var = float("inf"), float("inf")
    for i in torch.nonzero(deg >= 2).flatten().tolist():
        rows = torch.nonzero(dst == i).flatten()
        mi = m[rows]
        lo, hi = torch.sort(mi, 0).values, torch.sort(mi, 0, descending=True).values
        if i == R:                                                          # the designated bit-identical pair
            assert torch.equal(mi[0], mi[1])
            continue
        worst_gap = min(worst_gap, float((lo[1] - lo[0]).min()))
        if i == H:                                                          # the designated tie of the max: slots 63, 64
            assert torch.equal(m[names["h63"]], m[names["h64"]]) and torch.equal(hi[0], m[names["h63"]])
            assert torch.equal(hi[1], hi[0]) and torch.equal(lo[0], m[names["h256"]])
            worst_gap = min(worst_gap, float((hi[1] - hi[2]).min()))
        else:
            worst_gap = min(worst_gap, float((hi[0] - hi[1]).min()))
        var = (mi * mi).mean(0) - mi.mean(0) ** 2
        worst_var = min(worst_var, float(var.min()))
    print(f"   {what}: smallest gap {worst_gap:.3e} (needs >= {thr:.3e}), smallest variance {worst_var:.3e}")
    assert worst_gap >= thr, (what, worst_gap, thr)
    assert worst_var >= 1e-2, (what, worst_var)


def _oracle(a, b, t, ei, g_out, aggr, scal, dtype, skip=None):
    leaves = [None if v is None else v.detach().clone().to(dtype).requires_grad_(True) for v in (a, b, t)]
    out = PO.aggregate(leaves[0], leaves[1], leaves[2], ei, aggr, scal, AVG_DEG_LOG, skip)
    out.backward(g_out.to(dtype))
    res = {"out": out.detach(), "g_a": leaves[0].grad, "g_b": leaves[1].grad}
    if t is not None:
        res["g_t"] = leaves[2].grad                                         # (a removed edge's row: zeros)
    return res


def _hip(a, b, t, ei, g_out, aggr, scal, rel=None):
    rel = rel if rel is not None else Relation(ei.to(DEV), a.size(0), a.size(0), both=True)
    leaves = [None if v is None else v.detach().clone().to(DEV).requires_grad_(True) for v in (a, b, t)]
    out = Fh.PNAAggregateFn.apply(leaves[0], leaves[1], leaves[2], rel, aggr, scal, AVG_DEG_LOG)
    out.backward(g_out.to(DEV))
    res = {"out": out.detach(), "g_a": leaves[0].grad, "g_b": leaves[1].grad}
    if t is not None:
        res["g_t"] = leaves[2].grad
    assert int(rel.csr.flag.item()) == 0
    return res


# (case, F) -> seed: chosen on the CPU so that ``_preconditions`` holds (asserted in the test)
CASES = {"all": (ALL_AGGR, ALL_SCAL, True), "max": (("max",), ("identity",), True), "no_t": (ALL_AGGR, ALL_SCAL, False)}
SEEDS = {(c, F): 0 for c in CASES for F in WIDTHS}


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_operator_forward_and_gradients_under_the_float64_referee(case, F):
    aggr, scal, with_t = CASES[case]
    what = f"PNA aggregate {case} F={F}"
    ei, names, a, b, t, g = _inputs(F, SEEDS[(case, F)], with_t)
    _preconditions(a, b, t, ei, names, what)
    g_out = torch.randn(N_NODES, len(scal) * len(aggr) * F, generator=g)
    o32 = _oracle(a, b, t, ei, g_out, aggr, scal, torch.float32)
    o64 = _oracle(a, b, t, ei, g_out, aggr, scal, torch.float64)
    d64 = _oracle(a, b, t, ei, g_out, aggr, scal, torch.float64, skip=names["o"])   # O becomes an empty row
    got = _hip(a, b, t, ei, g_out, aggr, scal)
    assert got["out"].shape == (N_NODES, len(scal) * len(aggr) * F)
    referee_all(got, o32, o64, what)
    teeth(got, o32, o64, d64, what)
    # the empty row, exactly
    block = got["out"][Z].cpu().view(len(scal), len(aggr), F)
    for x, name in enumerate(aggr):
        if name != "std":
            assert bool((block[:, x] == 0).all()), name
    assert bool((got["g_a"][Z] == 0).all())


def test_two_backward_runs_agree_bit_for_bit():
    for F in (20, 260):
        ei, names, a, b, t, g = _inputs(F, 0)
        g_out = torch.randn(N_NODES, 15 * F, generator=g)
        rel = Relation(ei.to(DEV), N_NODES, N_NODES, both=True)
        first = _hip(a, b, t, ei, g_out, ALL_AGGR, ALL_SCAL, rel)
        again = _hip(a, b, t, ei, g_out, ALL_AGGR, ALL_SCAL, rel)
        for k in first:
            assert torch.equal(first[k], again[k]), (F, k)


def test_a_graph_gives_the_same_bits_first_and_last_in_a_batch():
    for F in (20, 260):
        ei, names, a, b, t, g = _inputs(F, 0)
        E = ei.size(1)
        g_out = torch.randn(N_NODES, 15 * F, generator=g)
        n2, e2 = 37, 150                                                    # a second graph, drawn
        ei2 = torch.randint(0, n2, (2, e2), generator=g)
        a2, b2, t2 = (torch.randn(n2, F, generator=g), torch.randn(n2, F, generator=g), torch.randn(e2, F, generator=g))
        go2 = torch.randn(n2, 15 * F, generator=g)
        first = _hip(torch.cat([a, a2]), torch.cat([b, b2]), torch.cat([t, t2]), torch.cat([ei, ei2 + N_NODES], 1),
                     torch.cat([g_out, go2]), ALL_AGGR, ALL_SCAL)
        last = _hip(torch.cat([a2, a]), torch.cat([b2, b]), torch.cat([t2, t]), torch.cat([ei2, ei + n2], 1),
                    torch.cat([go2, g_out]), ALL_AGGR, ALL_SCAL)
        for k in ("out", "g_a", "g_b"):
            assert torch.equal(first[k][:N_NODES], last[k][n2:]), (F, k)
            assert torch.equal(first[k][N_NODES:], last[k][:n2]), (F, k)
        assert torch.equal(first["g_t"][:E], last["g_t"][e2:]) and torch.equal(first["g_t"][E:], last["g_t"][:e2])


def test_on_a_tied_row_the_whole_of_g_max_lands_on_the_first_slot():
    F = 20
    ei, names, a, b, t, g = _inputs(F, 0)
    g_out = torch.randn(N_NODES, F, generator=g)
    got = _hip(a, b, t, ei, g_out, ("max",), ("identity",))
    first, second = sorted((names["r0"], names["r1"]))
    assert torch.equal(got["g_t"][first].cpu(), g_out[R]) and bool((got["g_t"][second] == 0).all())
    first, second = sorted((names["h63"], names["h64"]))                    # the tie across H's chunk boundary
    assert names["h63"] < names["h64"]
    assert torch.equal(got["g_t"][first].cpu(), g_out[H]) and bool((got["g_t"][second] == 0).all())
    got = _hip(a, b, t, ei, g_out, ("min",), ("identity",))
    assert torch.equal(got["g_t"][names["h256"]].cpu(), g_out[H])           # the argmin in the last chunk


def test_operand_checks():
    ei, names, a, b, t, g = _inputs(4, 0)
    rel = Relation(ei.to(DEV), N_NODES, N_NODES, both=True)
    ad, bd, td = a.to(DEV), b.to(DEV), t.to(DEV)
    with pytest.raises(TypeError, match="float32"):
        Fh.PNAAggregateFn.apply(ad.double(), bd, td, rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="contiguous"):
        Fh.PNAAggregateFn.apply(ad, bd.t().contiguous().t(), td, rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="edges"):
        Fh.PNAAggregateFn.apply(ad, bd, td[:-1], rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="avg_deg_log"):
        Fh.PNAAggregateFn.apply(ad, bd, td, rel, ("max",), ("amplification",))
    with pytest.raises(RuntimeError, match="CPU"):
        Fh.PNAAggregateFn.apply(a, b, t, rel, ("max",), ("identity",))
    one = Relation(ei.to(DEV), N_NODES, N_NODES)
    with pytest.raises(ValueError, match="both=True"):
        Fh.PNAAggregateFn.apply(ad, bd.clone().requires_grad_(True), td, one, ("max",), ("identity",))
    wide = torch.zeros(N_NODES, 513, device=DEV)
    with pytest.raises(ValueError, match="envelope"):
        Fh.PNAAggregateFn.apply(wide, wide, None, rel, ("max",), ("identity",))


# --------------------------------------------------------------------------- #
# the layer
# --------------------------------------------------------------------------- #
def _peptides(count=4, seed=0):
    graphs = make_dataset("peptides_func", count, seed=seed, edge_features=True)
    return graphs, Batch.from_data_list(graphs)


def _layer_run(ref, x, ei, ea, gy, dtype, skip=None):
    m = copy.deepcopy(ref).to(dtype)
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    out = m(xx, ei, None if ea is None else ea.to(dtype), skip)
    out.backward(gy.to(dtype))
    g = {"x.x": xx.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    return g, out.detach()


@pytest.mark.parametrize("edge", [True, False])
def test_pnaconv_against_its_twin_with_parameter_gradients(edge):
    graphs, b = _peptides()
    avg = PNAConfig.avg_deg_log_of(graphs)
    F, out_c, De = 12, 16, 3
    torch.manual_seed(3)
    ref = PO.PNAConvRef(F, out_c, ALL_AGGR, ALL_SCAL, avg, De if edge else None)
    prod = PNAConv(F, out_c, ALL_AGGR, ALL_SCAL, edge_dim=De if edge else None, avg_deg_log=avg).to(DEV)
    prod.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(b.num_nodes, F, generator=g)
    ea = b.edge_attr.float() + 0.25 * torch.randn(b.edge_attr.shape, generator=g) if edge else None
    gy = torch.randn(b.num_nodes, out_c, generator=g)
    what = f"PNAConv edge_dim={De if edge else None}"
    o32, y32 = _layer_run(ref, x, b.edge_index, ea, gy, torch.float32)
    o64, y64 = _layer_run(ref, x, b.edge_index, ea, gy, torch.float64)
    d64, dy64 = _layer_run(ref, x, b.edge_index, ea, gy, torch.float64, skip=int(b.edge_index.size(1)) // 2)
    xd = x.to(DEV).requires_grad_(True)
    y = prod(xd, b.edge_index.to(DEV), None if ea is None else ea.to(DEV))
    y.backward(gy.to(DEV))
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    teeth({"y": y}, {"y": y32}, {"y": y64}, {"y": dy64}, what)
    got = grads_of(prod, x=xd)
    assert all(v is not None for v in got.values())
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    assert {"x.x", "p.pre_nns.0.0.weight", "p.post_nns.0.0.weight", "p.lin.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what)


# --------------------------------------------------------------------------- #
# models
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("conv", ["pna", "pna_edge"])
def test_mpnn_pna_runs_at_the_graph_node_and_link_levels(conv):
    from graph_hscn import metrics
    from graph_hscn.loss import criterion
    from graph_hscn.train import batching
    from graph_hscn.train.train import eval_epoch
    cases = [("graph", "peptides_func", 9, 10, "cross_entropy"), ("node", "pascalvoc_sp_node", 14, 21, "weighted_cross_entropy"),
             ("link", "pcqm_contact_link", 9, 8, "cross_entropy")]
    for level, name, F, C, loss_fn in cases:
        graphs = make_dataset(name, 4, seed=0, edge_features=True)
        b = Batch.from_data_list(graphs)
        torch.manual_seed(0)
        pm = MPNN(CONV_DICT[conv], ACT_DICT["relu"], F, 16, C, 3, dropout=0.0, task_level=level,
                  pna=PNAConfig.from_graphs(graphs)).to(DEV)
        bd = batching.to_device(pm, b, DEV)
        pred, y = batching.forward(pm, bd)
        rows = {"graph": (4, C), "node": (b.num_nodes, C)}.get(level) or (b.edge_label_index.size(1),)
        assert tuple(pred.shape) == tuple(rows) and pm.last_engine == "layered"
        loss, _ = criterion(loss_fn, pred, y)
        loss.backward()
        assert np.isfinite(float(loss.detach()))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in pm.parameters()), (conv, level)
        if level == "link":
            l, perf = eval_epoch(0, None, DataLoader(graphs, 4), pm, loss_fn, None, "Test", link_metric="mrr")
        else:
            metric = metrics.eval_hip("ap" if level == "graph" else "f1_macro")
            l, perf = eval_epoch(0, None, DataLoader(graphs, 4), pm, loss_fn, metric, "Test")
        assert np.isfinite(l) and 0.0 <= perf <= 1.0


class _PNAGPSLayerRef(GPSO.GPSLayerRef):
    def __init__(self, D, heads, norm, cfg):
        super().__init__(D, "gcn", heads, norm)
        self.local_conv = "pna_edge"
        self.conv = PO.PNAConvRef(D, D, cfg.aggregators, cfg.scalers, cfg.avg_deg_log, D)

    def forward(self, x, edge_index, ptr, edge_attr=None, skip=None):
        h_a = self.norm1_attn(x + self.attn(x, ptr, skip))
        h_l = self.norm1_local(x + self.conv(x, edge_index, edge_attr))
        h = h_l + h_a
        f = self.ff_linear1(h)
        if self.watch is not None:
            self.watch("feed-forward hidden layer", f)
        return self.norm2(h + self.ff_linear2(torch.relu(f)))


GPS_D, GPS_HEADS, GPS_L = 16, 4, 2
GPS_SEED = 1        # chosen on the CPU: the float64 run keeps its ReLU inputs the required distance from zero (asserted)


def _gps_reference():
    from tests.test_gpu_attention import _Terms
    from tests.test_gpu_catenc import _Atom, _Bond
    graphs, b = _peptides(4, GPS_SEED)
    assert b.x.dtype == torch.int64 and b.edge_attr.dtype == torch.int64
    cfg = PNAConfig.from_graphs(graphs)
    torch.manual_seed(GPS_SEED)
    ref = GPSO.GPSRef(9, GPS_D, 10, GPS_L, GPS_HEADS, None, "layer", "graph")
    ref.layers = torch.nn.ModuleList(_PNAGPSLayerRef(GPS_D, GPS_HEADS, "layer", cfg) for _ in range(GPS_L))
    ref.node_encoder, ref.edge_encoder = _Atom(GPS_D), _Bond(GPS_D)
    gy = torch.randn(4, 10, generator=torch.Generator().manual_seed(1))

    def run(dtype, terms=False, skip=None, pool_skip=None):
        m = copy.deepcopy(ref).to(dtype)
        m.node_encoder.skip = m.edge_encoder.skip = None
        seen = {}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        tm = _Terms(m) if terms else None
        out = m(b.x, b.edge_index, m.edge_encoder(b.edge_attr), b.batch, b.ptr, 4, None, skip, pool_skip)
        out.backward(gy.to(dtype))
        if tm is not None:
            tm.close()
        g = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
        return g, out.detach(), seen, tm

    return cfg, b, ref, gy, run


def test_gps_pna_edge_with_atom_and_bond_encoders_under_the_float64_referee():
    from graph_hscn.train import batching
    from tests.test_gpu_attention import _check_gates
    what = "GPS local_conv=pna_edge + AtomEncoder + BondEncoder, graph level"
    cfg, b, ref, gy, run = _gps_reference()
    o32, y32, g32, _ = run(torch.float32)
    o64, y64, g64, terms = run(torch.float64, terms=True)
    _check_gates(g32, g64, what)
    key_drop, pool_drop = run(torch.float64, skip=(0, 0)), run(torch.float64, pool_skip=0)
    pm = GPS(9, GPS_D, 10, GPS_L, num_heads=GPS_HEADS, local_conv="pna_edge", activation=ACT_DICT["relu"], dropout=0.0,
             norm="layer", node_encoder="atom", edge_encoder="bond", pna=cfg).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    assert bd.x.dtype == torch.int64 and bd.edge_attr.dtype == torch.int64
    for layer in pm.layers:
        layer.conv.edge_encoder.materialize(GPS_D, bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": key_drop[1]}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values())
    # the two cancelling sums of tests/test_gpu_attention.py's model cases, named with their reasons there
    cancelling = [f"p.layers.{i}.attn.in_proj_bias" for i in range(GPS_L)] + [f"p.layers.{GPS_L - 1}.norm2.bias"]
    referee_all(got, o32, o64, what, terms=terms, cancelling=cancelling)
    terms.bound_teeth(got, o32, o64, [key_drop[0], pool_drop[0]], cancelling, what)
    reached = most_changed(o64, [key_drop[0]])
    assert {"p.node_encoder.weight", "p.edge_encoder.weight", "p.layers.0.conv.pre_nns.0.0.weight"} <= set(reached)
    teeth(got, o32, o64, {k: v for k, v in reached.items() if k not in cancelling}, what)
    pm.check_flags()


def test_a_few_training_steps_lower_a_finite_loss():
    from types import SimpleNamespace

    from graph_hscn import metrics
    from graph_hscn.train.train import eval_epoch, train
    graphs, b = _peptides(4, seed=0)
    torch.manual_seed(0)
    pm = build_mpnn(MPNNConfig("pna_edge", "relu", dropout=0.0, edge_encoder="bond", node_encoder="atom",
                               pna=PNAConfig.from_graphs(graphs)), 9, 10).to(DEV)
    metric_fn = metrics.eval_hip("ap")
    before, _ = eval_epoch(0, None, [b], pm, "cross_entropy", metric_fn, "Test")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", metric="ap", patience=10, min_delta=0.0)
    train(None, opt, cfg, [[b] * 5, [b], [b]], pm, metric_fn)
    after, _ = eval_epoch(1, None, [b], pm, "cross_entropy", metric_fn, "Test")
    assert np.isfinite(before) and np.isfinite(after) and after < before, (before, after)
    pm.check_flags()


def test_resident_entry_points_refuse_pna_by_name():
    from types import SimpleNamespace

    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    graphs, b = _peptides(4, seed=0)
    torch.manual_seed(0)
    pm = MPNN(CONV_DICT["pna_edge"], ACT_DICT["relu"], 9, 16, 10, 3, dropout=0.0).to(DEV)
    assert pm.resident_reason().startswith("convolution PNAConv")
    bd = batching.to_device(pm, b, DEV)
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(bd)
    assert pm.last_engine == "layered" and out.shape == (4, 10)
    pm.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="convolution PNAConv"):
        pm(bd)
    pm.engine = "layered"
    with pytest.raises(RuntimeError, match="convolution PNAConv"):
        MPNNResidentTrainStep(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="convolution PNAConv"):
        batching.resident_step(pm, bd, "cross_entropy")            # what replay.CapturedStep builds its step with
    with pytest.raises(RuntimeError, match="convolution PNAConv"):
        DeviceEvaluator(graphs, pm, "cross_entropy", 4).run()
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="convolution PNAConv"):
        fit_resident(None, opt, cfg, graphs, [], pm, 4)
