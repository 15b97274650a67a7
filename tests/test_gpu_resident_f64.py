"""The graph-resident launch pair (``hscn_resident_fwd`` / ``hscn_resident_bwd`` and their ``_with_virtual`` forms,
csrc/resident_kernels.h) THROUGH AUTOGRAD against the float64 referee of tests/test_gpu_layered_f64.py, at the sizes
where the kernels switch branch: the workgroup class (256 threads up to 64 nodes, else 1024), the register-parked
prologue loads and their tail loops (n H, the edge count, the head's H H + C H + C words), the two-buffer backward, the
forward's double-buffered weights and in-launch CSR export, the row tails of the 16-row MFMA tiles and 4-row chunks.

Harness: ``_check`` / ``_oracle_eval`` / ``multigraph`` / ``_randomise_biases`` of the layered file and
``helpers.referee_all`` / ``teeth`` / ``KinkGuard`` / ``TermMagnitudes`` with their constants as they stand:

    |HIP - f64|  <=  2 |oracle_f32 - f64| + 8 * 2^-23 * max|f64|          (per tensor, max norm)

No tolerance here is new and none is measured from the code under test.  The product side is
``HSCN("GAT", "GCN", "GCN")`` with ``engine = "resident"`` on a real ``HeteroBatch`` of hand-built graphs with explicit
cluster ids; the oracle is ``OM.HSCN`` with identical weights in float32 and float64.  Features are constants: only
parameter gradients are compared, with the oracle's ``None`` pattern for the virtual branch (it never reaches the
prediction).

Every case asserts: the resident engine ran and ``meta.check()``; through ``hscn_resident_launch_plan`` the branch the
case is named for (``expect``: numbers found on the host with that query and written down here, not computed at test
time); the prediction at 1e-5; the kink guard on the float64 oracle (the LOCAL output of every HeteroConv, ``lin_1``
under a ReLU head, pred - target under the L1 loss; the lv attention logits come with ``oracle_twin``); every gradient
through ``referee_all``; ``teeth`` against float64 references with one local -> local edge removed -- among the
candidates an edge into the last node of a graph and one into the first row of its last 16-row tile.  The referee run
is the one ``overlap_virtual = False`` makes (``hscn_resident_fwd`` + ``hscn_resident_bwd``, the pair the plan query
describes); the same step with ``overlap_virtual = True`` (the ``_with_virtual`` launches) must then be ``torch.equal``
in prediction and every gradient, so it stands under the same bar and the same teeth.

Teeth candidates: ``_drop_edges`` of the layered file over the batch's local -> local edges (all of them up to 48, else
an evenly spaced sample) with the two named ones added.

Seeds are fixed constants, chosen on the CPU so that the float64 oracle alone satisfies ``KinkGuard.check(1e-5, 1e-5)``
(at the large H = 32 shapes about one seed in three does); the assertion stays so that a change of seed or shape cannot
silently void the referee.

CANCELLING_LL_BIAS: only ``convs.*.local__to__local.bias`` -- a column sum of cotangents of both signs over all nodes,
the reason accepted in the layered file -- may be listed for a case, and only with ``bound_teeth`` passing (``_check``
does that for a listed case).  Any other tensor the referee rejects is a finding about the kernel.

Each case prints its plan, its referee lines and its worst ratio; profiles/resident_pair_f64_referee.txt records one
run.  Nothing is asserted from that file.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F_

from oracle import hetero_data as OH
from oracle import models as OM
from tests.helpers import ATOL, DEV, RTOL, close
from tests.test_gpu_layered_f64 import CANCELLING, _BIAS, _HL, _check, _drop_edges, _load, _randomise_biases, multigraph

pytestmark = pytest.mark.gpu

LL = ("local", "to", "local")


# --------------------------------------------------------------------------- #
# graphs
# --------------------------------------------------------------------------- #
def tree(n, seed, chords=None):
    """A random recursive tree on n nodes plus ``chords`` (default n // 8) random extra pairs, both directions of
    every pair: every node >= 1 has an in-edge, node n - 1 and the first row of the last 16-row tile among them."""
    g = torch.Generator().manual_seed(seed)
    if n < 2:
        return torch.zeros(2, 0, dtype=torch.long)
    par = (torch.rand(n - 1, generator=g) * torch.arange(1, n)).long()
    k = n // 8 if chords is None else chords
    a = torch.randint(0, n, (k,), generator=g)
    b = (a + 1 + torch.randint(0, n - 1, (k,), generator=g)) % n
    u, v = torch.cat([torch.arange(1, n), a]), torch.cat([par, b])
    return torch.stack([torch.cat([u, v]), torch.cat([v, u])])


def _graph(spec, seed):
    """spec = (kind, n[, arg]) -> (edge_index, cluster ids or None for random ones)."""
    kind, n = spec[0], spec[1]
    if kind == "tree":
        return tree(n, seed), None
    if kind == "dense":                      # spec[2] random pairs, both directions (repeats and all)
        return tree(n, seed, chords=spec[2] - (n - 1)), None
    if kind == "multi":
        return multigraph(n, seed), None
    if kind == "empty":                      # nodes, no edges
        return torch.zeros(2, 0, dtype=torch.long), None
    if kind == "onecluster":
        return tree(n, seed), np.full(n, 3)
    if kind == "clusters":                   # spec[2]: cluster sizes, ids (2 i + 1: not 0 .. U-1) shuffled over the nodes
        ids = np.concatenate([np.full(c, 2 * i + 1) for i, c in enumerate(spec[2])])
        assert ids.shape[0] == n
        return tree(n, seed), np.random.default_rng(seed).permutation(ids)
    raise KeyError(kind)


def build_batch(graphs, F, K, C, seed):
    """(oracle batch dict, product HeteroBatch on the CPU, [(offset, n)] per graph) from the graph specs."""
    from graph_hscn.data import Data, HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    data, ids = [], []
    for i, spec in enumerate(graphs):
        n = spec[1]
        ei, cid = _graph(spec, seed + 17 * i)
        data.append(Data(x=torch.randint(0, 5, (n, F), generator=g).float(), edge_index=ei, y=torch.zeros(1, C),
                         num_nodes=n))
        ids.append(rng.integers(0, K, n) if cid is None else cid)
    ob = OH.collate_hetero([OH.hetero_from_clusters(d.x, d.edge_index, d.y, i, K) for d, i in zip(data, ids)])
    pb = HeteroBatch.from_data_list([hetero_from_clusters(d, i, K) for d, i in zip(data, ids)])
    off = np.concatenate([[0], np.cumsum([s[1] for s in graphs])])
    return ob, pb, [(int(off[i]), s[1]) for i, s in enumerate(graphs)]


def named_edges(ei, spans):
    """Positions of an edge into the last node of a graph and of one into the first row of its last 16-row tile, from
    the largest graph that has both."""
    for o, n in sorted(spans, key=lambda s: -s[1]):
        last = torch.nonzero(ei[1] == o + n - 1).flatten()
        tile = torch.nonzero(ei[1] == o + 16 * ((n - 1) // 16)).flatten()
        if last.numel() and tile.numel():
            return [int(last[0]), int(tile[0])]
    raise AssertionError("no graph of the batch has an edge into its last node and into its last tile's first row")


# --------------------------------------------------------------------------- #
# the two sides
# --------------------------------------------------------------------------- #
class ORes(nn.Module):
    """The oracle on constant features; with ``loss`` the criterion's value (loss.py:6-19: mean BCE-with-logits / L1)
    in the dtype of the evaluation."""

    def __init__(self, m, loss=None):
        super().__init__()
        self.m, self.loss, self.l1_gate = m, loss, nn.Identity()

    def forward(self, xd, eis, batch_local, B, y=None):
        pred = self.m(xd, eis, batch_local, B)
        self.last_pred = pred.detach()
        if self.loss is None:
            return pred
        if self.loss == "l1":
            self.l1_gate(pred - y)           # |pred - y| has its kink where they meet
            return F_.l1_loss(pred, y)
        return F_.binary_cross_entropy_with_logits(pred, y, reduction="mean")


class PRes(nn.Module):
    """``HSCN`` on its HeteroBatch (the oracle's arguments are ignored: the batch is the same graphs).  ``loss``: the
    product criterion on the prediction -- its evaluation rides on the backward launch (``hscn_loss_tail``) unless
    ``read_loss`` reads the value first, which leaves the backward a ``LazyScaled`` gradient and its factor."""

    def __init__(self, m, loss=None, read_loss=False):
        super().__init__()
        self.m, self.loss, self.read_loss = m, loss, read_loss
        self.hb = self.y = None

    def forward(self, **_):
        from graph_hscn.loss import criterion
        pred = self.m(self.hb.x_dict, self.hb.edge_index_dict, self.hb)
        self.last_pred = pred.detach()
        if self.loss is None:
            return pred
        loss, _score = criterion(self.loss, pred, self.y)
        if self.read_loss:
            float(loss)
        return loss


class _LocalOut:
    """``KinkGuard.relu_after`` on the LOCAL rows of a HeteroConv's output (the virtual rows feed no gradient)."""

    def __init__(self, conv):
        self.conv = conv

    def register_forward_hook(self, fn):
        return self.conv.register_forward_hook(lambda m, a, out: fn(m, a, out["local"]))


def _gates(act, loss):
    def gates(m):
        g = [_LocalOut(c) for c in m.m.convs]
        if act == "relu":
            g.append(m.m.lin_1)
        if loss == "l1":
            g.append(m.l1_gate)
        return g
    return gates


# --------------------------------------------------------------------------- #
# cases.  sizes: nodes per graph of the one batch; a plain int is ("tree", n).
# expect: fields of hscn_resident_launch_plan for the batch's maxima, found with the query on the host.
# --------------------------------------------------------------------------- #
def case(id, H, L, sizes, F=9, C=3, K=8, act="relu", loss=None, read_loss=False, seed=1, **expect):
    graphs = [s if isinstance(s, tuple) else ("tree", s) for s in sizes]
    return pytest.param(dict(id=id, H=H, L=L, F=F, C=C, K=K, act=act, loss=loss, read_loss=read_loss, graphs=graphs,
                             seed=seed, expect=expect), id=id)


S256 = (1, 2, 15, 16, 17, 33, 63, 64)
CASES = [
    # ---- 256-thread class (NW = 4 waves)
    case("t256-H16-L3", 16, 3, S256, threads=256, db=1, exp=1, two=0),
    case("t256-H32-L2-nH2048", 32, 2, S256, threads=256, db=1, exp=1, two=0, seed=2),
    # 16 weight-gradient tiles on 4 waves (four passes of the fold), the prologue tail beyond n = 32, and with L = 2 the
    # non-MFMA input gradient of layer 1
    case("t256-H64-L2-four-pass-fold", 64, 2, (1, 31, 32, 33, 64), threads=256, db=0, exp=1, two=0),
    # ---- 1024-thread class (NW = 16)
    case("t1024-H16-65-beside-64", 16, 3, (64, 65), threads=1024, db=1, exp=1, two=0),
    case("t1024-H16-L3", 16, 3, (65, 127, 128, 129, 257), threads=1024, db=1, exp=1, two=0, seed=2),
    case("t1024-H32-L2-nH8192", 32, 2, (255, 256, 257), threads=1024, db=1, exp=1, two=0, seed=4),
    case("t1024-H64-L2-65-beside-64", 64, 2, (64, 65), threads=1024, db=0, exp=1, two=0, seed=5),
    # n = 117 with this generator's 260 edges is the last graph the H = 64 plan accepts (118: unsupported)
    case("t1024-H64-L2-largest-n117", 64, 2, (40, 117), threads=1024, db=0, exp=0, csr_launch=1, two=0),
    # ---- buffers, H = 32: three n x H buffers fit up to n = 337 (758 edges), two from 338; the buffers swap roles once
    # per layer, so each at an even and an odd number of layers
    case("H32-L2-two0-n337", 32, 2, (40, 337), threads=1024, db=1, exp=1, two=0),
    case("H32-L3-two0-n337", 32, 3, (40, 337), threads=1024, db=1, exp=1, two=0, seed=2),
    case("H32-L2-two1-n338", 32, 2, (40, 338), threads=1024, db=1, exp=1, two=1),
    case("H32-L3-two1-n338", 32, 3, (40, 338), threads=1024, db=1, exp=1, two=1),
    # single-buffered weights from n = 385; the in-launch CSR export fits up to n = 439, from 440 k_ll_csr_t builds it
    case("H32-L2-db0-n385", 32, 2, (40, 385), threads=1024, db=0, exp=1, csr_launch=0, two=1),
    case("H32-L2-exp1-n439", 32, 2, (40, 439), threads=1024, db=0, exp=1, csr_launch=0, two=1),
    case("H32-L2-exp0-n440-csr-launch", 32, 2, (40, 440), threads=1024, db=0, exp=0, csr_launch=1, two=1, seed=4),
    # ---- edge tails: more edges in one graph than EPT * RT parks in registers (512 at 256 threads, 2048 at 1024)
    case("edges-600-on-64-nodes", 16, 2, (17, ("dense", 64, 300)), threads=256, ell_over=512),
    case("edges-2200-on-200-nodes", 16, 2, (17, ("dense", 200, 1100)), threads=1024, ell_over=2048),
    # ---- head: HT = H H + C H + C words against 2 RT parked ones switches between C = 15 / 16 (H = 16, 256 threads)
    # and C = 31 / 32 (H = 32, 1024 threads); every head activation once
    case("head-H16-t256-C15-relu", 16, 2, (17, 64), C=15, act="relu", threads=256, seed=2),
    case("head-H16-t256-C16-elu", 16, 2, (17, 64), C=16, act="elu", threads=256, seed=2),
    case("head-H32-t1024-C31-tanh", 32, 2, (17, 65), C=31, act="tanh", threads=1024, seed=3),
    case("head-H32-t1024-C32-identity", 32, 2, (17, 65), C=32, act="identity", threads=1024, seed=3),
    case("head-C1", 16, 2, (17, 33), C=1, threads=256),
    # ---- the loss riding on the backward launch (hscn_loss_tail), and read first (LazyScaled and its factor)
    case("loss-tail-cross-entropy", 16, 3, (15, 33, 64), C=10, loss="cross_entropy", threads=256, seed=2),
    case("loss-tail-l1", 32, 2, (17, 65, 129), C=11, loss="l1", threads=1024, seed=3),
    case("loss-read-first-lazy-scaled", 16, 3, (15, 33, 64), C=10, loss="cross_entropy", read_loss=True, threads=256, seed=2),
    # ---- input widths
    case("F1-H16", 16, 2, (16, 33, 70), F=1, threads=1024),
    case("F9-H16", 16, 2, (16, 33, 70), F=9, threads=1024, seed=2),
    case("F16-H16", 16, 2, (16, 33, 70), F=16, threads=1024),
    case("F1-H32", 32, 2, (16, 33, 70), F=1, threads=1024),
    case("F9-H32", 32, 2, (16, 33, 70), F=9, threads=1024),
    case("F32-H32", 32, 2, (16, 33, 70), F=32, threads=1024),
    # ---- structure: a hub of in-degree > 64, repeated edges, input self loops, isolated nodes, one-way edges
    case("multigraph-17", 16, 3, (("multi", 17), 20), threads=256),
    case("multigraph-129", 16, 3, (("multi", 129), 40), threads=1024),
    case("no-edges-and-one-cluster", 16, 3, (("empty", 5), ("onecluster", 7), 1, 20, 2), threads=256),
]


def build_case(c):
    """Everything of a case that needs no device: (oracle wrapper, product wrapper on the CPU, product batch, consts,
    cotangent, dropped-edge consts, plan)."""
    from graph_hscn import _hip
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    H, L, F, C, K, seed = c["H"], c["L"], c["F"], c["C"], c["K"], c["seed"]
    ob, pb, spans = build_batch(c["graphs"], F, K, C, seed)
    B = len(c["graphs"])
    torch.manual_seed(seed)
    om = _randomise_biases(ORes(OM.HSCN("GAT", "GCN", "GCN", OM.ACT[c["act"]], F, H, C, L), c["loss"]), seed, 0.1)
    pm = PRes(HSCN("GAT", "GCN", "GCN", ACT_DICT[c["act"]], F, H, C, L), c["loss"], c["read_loss"])
    g = torch.Generator().manual_seed(seed + 1)
    consts = {"xd": ob["x_dict"], "eis": ob["edge_index_dict"], "batch_local": ob["batch_local"], "B": B}
    if c["loss"] is None:
        gy = torch.randn(B, C, generator=g)
    else:
        gy = torch.tensor(0.7)               # the factor the backward launch applies (g_scale)
        consts["y"] = (torch.rand(B, C, generator=g) > 0.5).float() if c["loss"] == "cross_entropy" \
            else torch.randn(B, C, generator=g)
    eis = ob["edge_index_dict"]
    drops = [dict(consts, eis={**eis, LL: e}) for (e,) in _drop_edges(eis[LL], must=named_edges(eis[LL], spans))]
    maxima = (int(pb["local"].max_nodes), int(pb["virtual"].max_nodes), int(pb[LL].max_edges),
              int(pb[("virtual", "to", "virtual")].max_edges))
    plan = _hip.resident_launch_plan(F, H, L, C, *maxima, True)
    return om, pm, pb, consts, gy, drops, maxima, plan


def run_case(c):
    from graph_hscn import engine
    what = "resident " + c["id"]
    om, pm, pb, consts, gy, drops, maxima, plan = build_case(c)
    print(f"[resident f64] {what}: (max_n, max_v, max_ell, max_evv) = {maxima} plan = {plan}")
    assert plan is not None, "the resident launches take this batch"
    expect = dict(c["expect"])
    ell_over = expect.pop("ell_over", None)
    assert ell_over is None or maxima[2] > ell_over, f"{what}: {maxima[2]} edges, the case needs more than {ell_over}"
    for k, v in expect.items():
        assert plan[k] == v, f"{what}: the plan's {k} is {plan[k]}, the case is named for {v}"
    pm = _load(pm, om)
    pm.hb = pb.to(DEV)
    if "y" in consts:
        pm.y = consts["y"].to(DEV)
    pm.m.engine, pm.m.keep_virtual, pm.m.overlap_virtual = "resident", False, False
    worst, (o32, g32, o64, g64, od, gd) = _check(what, om, pm, {}, consts, gy, gates=_gates(c["act"], c["loss"]),
                                                 atol=ATOL, rtol=RTOL, drops=drops,
                                                 chain_extra=int(consts["batch_local"].numel()))
    assert pm.m.last_engine == "resident"
    pm.hb._resident_meta.check()
    pred = pm.last_pred.clone()
    if c["loss"] is not None:                # ``_check`` compared the loss: the prediction behind it
        with torch.no_grad():
            om(**consts)
        assert close(pred, om.last_pred, atol=ATOL, rtol=RTOL), f"{what}: prediction outside the bar"
    # the same step with the virtual branch riding on both launches: bit for bit
    pm.m.overlap_virtual = True
    engine.last_deferred_virtual = None
    pm.zero_grad(set_to_none=True)
    out = pm()
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    pm.hb._resident_meta.check()
    assert pm.m.last_engine == "resident"
    assert engine.last_deferred_virtual is not None, f"{what}: the virtual branch did not ride on the backward launch"
    assert torch.equal(pm.last_pred, pred), f"{what}: prediction differs with overlap_virtual"
    for n_, p in pm.named_parameters():
        k = "p." + n_
        if gd[k] is None:
            assert p.grad is None, k
        else:
            assert p.grad is not None and torch.equal(p.grad, gd[k]), f"{what} {k}: differs with overlap_virtual"
    print(f"   overlap_virtual: prediction and {sum(v is not None for v in gd.values())} gradients bit-identical")
    return worst




# The (case, tensor) pairs that may take helpers.TermMagnitudes' a-priori bound where the referee rejects them.  Only a
# local -> local convolution bias may stand here -- a column sum of cotangents of both signs over all nodes, the reason
# accepted in the layered file -- and ``_check`` then demands ``bound_teeth`` for it: a float64 reference with one edge
# removed must be rejected by referee and bound together.  {case id: layers whose ll bias is listed}
CANCELLING_LL_BIAS = {}
CANCELLING.update({"resident " + k: {_HL % (l, "bias"): _BIAS for l in layers} for k, layers in CANCELLING_LL_BIAS.items()})


@pytest.mark.parametrize("c", CASES)
def test_resident_pair_against_the_float64_referee(c):
    run_case(c)


# --------------------------------------------------------------------------- #
# the virtual branch: it never reaches the prediction, so no gradient above sees it.  Its final features against
# float64 under the bar tests/test_gpu_resident.py::test_hip_is_as_close_to_float64_as_the_float32_oracle states:
#     |HIP - f64| <= |oracle32 - f64| + 4 ulp(scale),      ulp(scale) = 2^-23 max(1, max|f64|)
# at the edges of the lv softmax's chunks of 64 members.
# --------------------------------------------------------------------------- #
def _virtual_features(m, xd, eis, dtype):
    x = {k: v.to(dtype) for k, v in xd.items()}
    with torch.no_grad():
        for conv in m.convs:
            x = {k: v.relu() for k, v in conv(x, eis).items()}
    return x["virtual"].double()


def _virtual_bar(hip, r32, r64):
    e_hip, e_o32 = float((hip - r64).abs().max()), float((r32 - r64).abs().max())
    ulp = 2.0 ** -23 * max(1.0, float(r64.abs().max()))
    return e_hip, e_o32 + 4 * ulp


CHUNK_EDGES = (1, 63, 64, 65, 128, 129)


@pytest.mark.parametrize("id,H,L,K,graphs", [
    ("chunk-edges-H16-L3", 16, 3, 8, [("clusters", 450, CHUNK_EDGES), ("tree", 20)]),
    ("chunk-edges-H32-L2", 32, 2, 8, [("clusters", 450, CHUNK_EDGES), ("tree", 20)]),
    ("K1-on-257-nodes", 16, 2, 1, [("clusters", 257, (257,))]),
    ("two-of-eight-cluster-ids", 16, 2, 8, [("clusters", 40, (25, 15)), ("tree", 9)]),
])
def test_virtual_features_at_the_attention_chunk_edges(id, H, L, K, graphs):
    import copy
    from graph_hscn import _hip, engine
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    F, C, seed = 9, 3, 5
    ob, pb, spans = build_batch(graphs, F, K, C, seed)
    B = len(graphs)
    LV = ("local", "to", "virtual")
    eis, xd = ob["edge_index_dict"], ob["x_dict"]
    members = torch.bincount(eis[LV][1], minlength=xd["virtual"].size(0))
    n0 = graphs[0][1]
    assert sorted(members[: len(graphs[0][2])].tolist()) == sorted(graphs[0][2]), "the clusters have the sizes named"
    torch.manual_seed(seed)
    om = _randomise_biases(OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L), seed, 0.1)
    pm = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L).to(DEV)
    pm.load_state_dict(om.state_dict())
    maxima = (int(pb["local"].max_nodes), int(pb["virtual"].max_nodes), int(pb[LL].max_edges),
              int(pb[("virtual", "to", "virtual")].max_edges))
    plan = _hip.resident_launch_plan(F, H, L, C, *maxima, True)
    print(f"[resident f64] virtual {id}: (max_n, max_v, max_ell, max_evv) = {maxima} cluster sizes = "
          f"{members.tolist()} plan = {plan}")
    assert plan is not None
    r32 = _virtual_features(om, xd, eis, torch.float32)
    o64 = copy.deepcopy(om).double()
    r64 = _virtual_features(o64, xd, eis, torch.float64)
    hb = pb.to(DEV)
    V = r64.size(0)
    got = {}
    pm.engine, pm.keep_virtual, pm.overlap_virtual = "resident", True, False
    pm(hb.x_dict, hb.edge_index_dict, hb)
    got["last_virtual"] = pm.last_virtual[:V].detach().cpu().double()
    pm.keep_virtual, pm.overlap_virtual = False, True
    engine.last_deferred_virtual = None
    pm(hb.x_dict, hb.edge_index_dict, hb).sum().backward()
    torch.cuda.synchronize()
    assert pm.last_engine == "resident" and engine.last_deferred_virtual is not None
    hb._resident_meta.check()
    got["last_deferred_virtual"] = engine.last_deferred_virtual[:V].detach().cpu().double()
    assert torch.equal(got["last_virtual"], got["last_deferred_virtual"])
    for k, hip in got.items():
        e, lim = _virtual_bar(hip, r32, r64)
        print(f"   virtual {id} {k}: |HIP-f64| = {e:.3e}  limit = {lim:.3e}  ratio = {e / lim:.3f}")
        assert e <= lim, (k, e, lim)
    if 65 not in graphs[0][2]:
        return
    # teeth: the 65-member cluster without the one member of its second chunk of 64 (its last lv edge: the CSR keeps
    # the edge order) -- the same bar must reject that reference
    v65 = int(torch.nonzero(members[: len(graphs[0][2])] == 65).flatten()[0])
    e65 = torch.nonzero(eis[LV][1] == v65).flatten()
    assert e65.numel() == 65 and int(e65[-1]) < n0
    keep = torch.ones(eis[LV].size(1), dtype=torch.bool)
    keep[e65[64]] = False
    q64 = _virtual_features(o64, xd, {**eis, LV: eis[LV][:, keep].contiguous()}, torch.float64)
    for k, hip in got.items():
        e, lim = _virtual_bar(hip, r32 - r64 + q64, q64)
        print(f"   virtual {id} {k} [one member dropped]: |HIP-f64| = {e:.3e}  limit = {lim:.3e}")
        assert e > lim, f"{k}: the bar cannot see a member missing from the second chunk"


# --------------------------------------------------------------------------- #
# differentiable feature inputs: the resident launches return parameter gradients only
# --------------------------------------------------------------------------- #
def test_feature_gradients_route_auto_to_the_layered_engine():
    """A batch the resident engine takes, with ``x_local.requires_grad_()`` (a trainable node encoder in front of the
    model): ``engine="auto"`` must return the input gradient -- through the layered operators -- and it passes the
    referee against the oracle's; ``engine="resident"`` must refuse and say why; half storage with a differentiable
    input raises on either setting."""
    import copy
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    from tests.helpers import referee
    F, H, L, C, K, seed = 9, 16, 3, 3, 8, 3
    graphs = [("tree", n) for n in (15, 33, 64, 70)]
    ob, pb, _ = build_batch(graphs, F, K, C, seed)
    B = len(graphs)
    torch.manual_seed(seed)
    om = _randomise_biases(OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L), seed, 0.1)
    pm = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L).to(DEV)
    pm.load_state_dict(om.state_dict())
    gy = torch.randn(B, C, generator=torch.Generator().manual_seed(seed + 1))
    ref = {}
    for dt, m in ((torch.float32, om), (torch.float64, copy.deepcopy(om).double())):
        x = {k: v.detach().clone().to(dt) for k, v in ob["x_dict"].items()}
        x["local"].requires_grad_()
        m(x, ob["edge_index_dict"], ob["batch_local"], B).backward(gy.to(dt))
        ref[dt] = x["local"].grad
    hb = pb.to(DEV)
    pm.engine = "auto"
    with torch.no_grad():
        pm(hb.x_dict, hb.edge_index_dict, hb)
    assert pm.last_engine == "resident", "the batch qualifies for the resident engine"
    pm(hb.x_dict, hb.edge_index_dict, hb).backward(gy.to(DEV))
    assert pm.last_engine == "resident"
    g_resident = {n_: p.grad.clone() for n_, p in pm.named_parameters() if p.grad is not None}
    pm.zero_grad(set_to_none=True)
    xl = hb.x_dict["local"].detach().clone().requires_grad_()
    pm(dict(hb.x_dict, local=xl), hb.edge_index_dict, hb).backward(gy.to(DEV))
    assert pm.last_engine == "layered"
    assert xl.grad is not None, "engine='auto' returns the gradient of a differentiable feature input"
    print("[resident f64] feature gradients")
    assert referee(xl.grad, ref[torch.float32], ref[torch.float64], "x_local through engine='auto'") <= 1.0
    assert g_resident.keys() == {n_ for n_, p in pm.named_parameters() if p.grad is not None}
    pm.engine = "resident"
    with pytest.raises(RuntimeError, match="require grad"):
        pm(dict(hb.x_dict, local=xl), hb.edge_index_dict, hb)
    with torch.no_grad():                      # nothing to differentiate: the resident engine takes the same tensors
        pm(dict(hb.x_dict, local=xl), hb.edge_index_dict, hb)
    assert pm.last_engine == "resident"
    half = {k: v.half() for k, v in hb.x_dict.items()}
    half["local"].requires_grad_()
    for eng in ("auto", "resident"):
        pm.engine = eng
        with pytest.raises(RuntimeError, match="half-precision node features that require grad"):
            pm(half, hb.edge_index_dict, hb)


def test_scn_feature_gradients_route_forward_graphs_to_the_layered_operators():
    """``SCN.forward_graphs`` on a graph its fused launch takes: with ``data.x.requires_grad_()`` it runs the layered
    operators and returns the input gradient, which passes the referee against the oracle's stage-A body."""
    import copy
    from graph_hscn.data import Batch, Data
    from graph_hscn.model.hscn import SCN
    from tests.helpers import referee, scn_step_in_dtype
    n, F, K, seed = 57, 9, 4, 6
    ei = tree(n, seed)
    x = torch.randint(0, 5, (n, F), generator=torch.Generator().manual_seed(seed)).float()
    torch.manual_seed(seed)
    om = OM.SCN([16], "elu", F, K)
    pm = SCN([16], "elu", F, K, mincut_route="sparse").to(DEV)
    pm.load_state_dict(om.state_dict())
    ref = {}
    for dt, m in ((torch.float32, om), (torch.float64, copy.deepcopy(om).double())):
        xx = x.detach().clone().to(dt).requires_grad_()
        _, mc, o = scn_step_in_dtype(m, xx, ei)
        (mc + o).backward()
        ref[dt] = xx.grad
    data = Batch.from_data_list([Data(x=x, edge_index=ei, num_nodes=n)]).to(DEV)
    _, mc, o = pm.forward_graphs(data)
    assert pm.last_engine == "resident", "the graph qualifies for the fused stage-A launch"
    data.x = data.x.detach().clone().requires_grad_()
    _, mc, o = pm.forward_graphs(data)
    assert pm.last_engine == "layered"
    (mc + o).backward()
    assert data.x.grad is not None
    print("[resident f64] SCN feature gradients")
    assert referee(data.x.grad, ref[torch.float32], ref[torch.float64], "x through SCN.forward_graphs") <= 1.0
    data.x = data.x.detach().half().requires_grad_()
    with pytest.raises(RuntimeError, match="half-precision features that require grad"):
        pm.forward_graphs(data)
