"""Stage A graph-resident (csrc/resident_scn.hip: ``k_scn_fwd`` / ``k_scn_bwd`` under autograd, ``k_scn_step`` through
``ScnTrainStep(one_launch=True)``) against the float64 referee of tests/test_gpu_layered_f64.py, on graphs chosen for
the kernels' own branch edges: the 16-row MFMA tiles and 4-row chunks, the second tile a wave takes from n = 257, the
``GSCR`` = 4096-word threshold of ``scn_layout`` (which dead buffer the Gram scratch reuses), the register windows of
``scn_front`` (8192 feature words, 2048 edges) and the loops behind them, the 16-column tiles of S (``gram_mfma`` from
K > 16, a 4-column last tile, the scalar branches at K % 4 != 0), one-way edges (the step's (A + A^T) S walks both
CSRs), a hub, repeated edges, input self loops, isolated nodes, E = 0, B = 1, F = 1 and F = 16.

Harness: ``OSCN`` / ``_load`` / ``_references`` / ``_judge`` / ``_check`` / ``_drop_edges`` / ``multigraph`` of the layered
file, ``tree`` of tests/test_gpu_resident_f64.py, ``helpers.referee_all`` / ``teeth`` / ``KinkGuard`` with their constants
as they stand:

    |HIP - f64|  <=  2 max_r |oracle_f32_r - f64| + 8 * 2^-23 * max|f64|          (per tensor, max norm)

The yardstick is taken over EIGHT float32 evaluations of the CPU oracle ``OSCN``: the batch as given and seven
relabelled copies (``helpers.relabel_graphs``, seeds ``YARDSTICK_SEEDS``: per graph a node permutation and a shuffled
edge order -- the same gradients in exact arithmetic, another summation order).  MinCUT gradients are sums that cancel
and a single float32 evaluation's distance to float64 is a noisy draw of it: held to one draw, a relabelled float32
oracle evaluation -- a correct evaluation by construction -- is rejected about one time in ten; over eight draws none
of 1 485 was.  The yardstick is measured on the reference alone, never on HIP output;
tests/test_stage_a_referee_host.py shows without a GPU that four further, held-out relabelled evaluations pass this bar
in every case below and are rejected against a reference with one edge removed.

Every case asserts, per engine (the launch pair under autograd; for A .. J also the one-launch step): the engine that
ran and ``meta.check()``; S and both losses within ATOL / RTOL of the float32 oracle; the kink guard on the float64
oracle (ReLU cases: seeds are constants chosen on the CPU so that it holds); all five gradients through the eight-draw
``referee_all`` with the layered file's ``chain_extra``; ``teeth`` against float64 references with one edge of the
largest graph removed -- ``_drop_edges`` with an edge into that graph's last node and one into the first row of its
last 16-row tile among the candidates where the graph has them (``multigraph`` isolates its last nodes: the hub's
edges instead).  Then: the step's S and losses ``torch.equal`` to the pair's; both engines repeat with identical bits;
with a ``ScnStructurePool`` the step's second run (structure loaded through the cached front) ``torch.equal`` to its
first.  P1 .. P5 lie outside the step's envelope: ``ScnTrainStep(one_launch=True)`` raises, the query answers 0,
nothing is launched.  The sizes of a case decide its branch: ``max_n`` / ``max_e`` are the batch's own maxima.

``expect``: what ``hscn_scn_resident_supported`` / ``hscn_scn_resident_train_step_supported`` answer for the case's
(F, H, K, max_n, max_e), and where named the largest n they accept at the case's max_e -- found with the queries on the
host and written down here; tests/test_stage_a_referee_host.py asserts them.

CANCELLING: a (case, tensor) pair may take ``helpers.TermMagnitudes``' a-priori bound only with the reason ``_MINCUT``
and only for ``mlp.0.*``, ``lin_rel.*`` or ``lin_root.weight``, with ``bound_teeth`` passing (``_judge`` demands it).
Any other rejection is a finding about the kernel.

Each case prints its referee lines and worst ratios; profiles/scn_resident_f64_referee.txt records one run.  Nothing is
asserted from that file.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import models as OM
from tests.helpers import ATOL, DEV, RTOL, relabel_graphs
from tests.test_gpu_layered_f64 import (CANCELLING, OSCN, _MINCUT, _check, _drop_edges, _hub_edges, _judge, _load,
                                        _references, _scn_gates, multigraph)
from tests.test_gpu_resident_f64 import tree

pytestmark = pytest.mark.gpu

YARDSTICK_SEEDS = (101, 102, 103, 104, 105, 106, 107)      # the seven relabelled copies behind the yardstick
HELD_OUT_SEEDS = (201, 202, 203, 204)                       # tests/test_stage_a_referee_host.py: never in the yardstick


# --------------------------------------------------------------------------- #
# graphs
# --------------------------------------------------------------------------- #
def one_way(ei, seed):
    """``_scn_graphs``' rule of the layered file: a third of the edges with src < dst dropped, so that about a third
    of the pairs keep one direction only."""
    rng = np.random.default_rng(seed)
    keep = torch.from_numpy(rng.random(ei.size(1)) > 0.33) | (ei[0] > ei[1])
    return ei[:, keep].contiguous()


def _edges(spec, seed):
    kind, n = spec[0], spec[1]
    if kind == "oneway":
        return one_way(tree(n, seed), seed)
    if kind == "sym":
        return tree(n, seed)
    if kind == "dense":                      # spec[2] chords on the tree, both directions, repeats and all
        return tree(n, seed, chords=spec[2])
    if kind == "multi":
        return multigraph(n, seed)
    if kind == "empty":
        return torch.zeros(2, 0, dtype=torch.long)
    raise KeyError(kind)


def build_graphs(c):
    """[(x float32 [n, F] of randint(0, 5), edge_index int64 [2, e])] of a case."""
    g = torch.Generator().manual_seed(c["seed"])
    return [(torch.randint(0, 5, (s[1], c["F"]), generator=g).float(), _edges(s, c["seed"] + 17 * i))
            for i, s in enumerate(c["graphs"])]


def named_candidates(ei, n, kind):
    """Edge positions that must be among the teeth's candidates: an edge into the last node and one into the first row
    of the last 16-row tile (``multigraph`` leaves its last tenth of the nodes isolated: the hub's first edges)."""
    if kind == "multi":
        return _hub_edges(ei)
    must = []
    for node in (n - 1, 16 * ((n - 1) // 16)):
        hit = torch.nonzero(ei[1] == node).flatten()
        if hit.numel():
            must.append(int(hit[0]))
    return sorted(set(must))


# --------------------------------------------------------------------------- #
# cases.  sizes: nodes per graph; ``kind`` the generator of every graph unless a size is a (kind, n[, arg]) tuple.
# expect: pair / step = the two queries' answers for the batch's maxima; pair_max_n / step_max_n = the largest max_n the
# query accepts at the case's max_e.
# --------------------------------------------------------------------------- #
def case(id, sizes, K, H, act, kind, F, seed=1, **expect):
    graphs = [s if isinstance(s, tuple) else (kind, s) for s in sizes]
    return pytest.param(dict(id=id, K=K, H=H, act=act, F=F, graphs=graphs, seed=seed, expect=expect), id=id)


CASES = [
    # row and chunk tails of the 16-row tiles; the one-node graph has no edge
    case("A-row-tails-K4-F1", (1, 2, 15, 16, 17), 4, 16, "elu", "oneway", 1, pair=1, step=1),
    # n K = n H = 4096 = GSCR at n = 256; a wave's second tile from n = 257
    case("B-gscr-256-second-tile", (255, 256, 257), 16, 16, "relu", "oneway", 9, pair=1, step=1),
    # B = 1: the workgroup writes the gradients, no fold; both tiles of every wave; 512 * 16 feature words fill the
    # register window exactly; F = FP: no padding
    case("C-n512-B1-F16", (512,), 16, 16, "elu", "oneway", 16, pair=1, step=1),
    # n H = 4096 at n = 128 (H = 32); K = 8 half fills the column tile
    case("D-gscr-128-H32-K8", (127, 128, 129), 8, 32, "tanh", "sym", 9, pair=1, step=1),
    # two column tiles (gram_mfma), a second row tile, near the step's K = 32 envelope
    case("E-K32-two-column-tiles", (353, 31), 32, 16, "elu", "oneway", 9, pair=1, step=1, step_max_n=372),
    # H = 32 (TD = 2) near its envelope
    case("F-H32-n420", (420, 6), 16, 32, "identity", "oneway", 9, pair=1, step=1, step_max_n=430),
    # a hub of in-degree > 64, repeated edges, input self loops, isolated nodes; F = 13; B = 1
    case("G-multigraph-K12-F13", (33,), 12, 16, "relu", "multi", 13, pair=1, step=1),
    # 2 378 edges on 90 nodes: beyond the 2 048-edge register window
    case("H-2378-edges", (("dense", 90, 1100), ("sym", 9)), 16, 16, "elu", "sym", 9, pair=1, step=1),
    # K = 20: a 4-column last tile (with these 75 edges the step's limit is its 512-node cap, not the LDS)
    case("I-K20-last-tile-4", (40, 7), 20, 16, "tanh", "oneway", 9, pair=1, step=1, step_max_n=512),
    # E = 0: edge_index is passed as NULL; B = 1
    case("J-no-edges", (("empty", 4),), 4, 16, "elu", "empty", 9, pair=1, step=1),
    # ---- pair only: outside the one-launch step's envelope
    case("P1-n513-n600", (513, 600), 16, 16, "elu", "oneway", 9, pair=1, step=0, pair_max_n=634),   # max_n > 512
    case("P2-K5-scalar-paths", (33, 16), 5, 16, "elu", "oneway", 9, pair=1, step=0),                 # K % 4 != 0
    case("P3-K64-four-column-tiles", (65,), 64, 16, "tanh", "sym", 9, pair=1, step=0),              # K > 32
    case("P4-H32-K32", (129,), 32, 32, "relu", "oneway", 9, pair=1, step=0),                         # NT * TD = 4
    case("P5-multigraphs-K6", (40, 7, 129), 6, 16, "elu", "multi", 9, pair=1, step=0),               # K % 4 != 0
]


def what_of(c):
    return "SCN resident " + c["id"]


# (case, tensor) pairs that may take the a-priori bound where the referee rejects them: reason _MINCUT only, tensors
# mlp.0.* / lin_rel.* / lin_root.weight only, and ``bound_teeth`` must pass for them
CANCELLING_MINCUT = {}
for _id, _keys in CANCELLING_MINCUT.items():
    assert all(k.split("p.m.")[1] in ("mlp.0.weight", "mlp.0.bias", "mp.module_0.lin_rel.weight",
                                      "mp.module_0.lin_rel.bias", "mp.module_0.lin_root.weight") for k in _keys)
    CANCELLING["SCN resident " + _id] = {k: _MINCUT for k in _keys}


def build_case(c):
    """Everything of a case that needs no device: (oracle wrapper, graphs, maxima, consts, drops, draws, chain_extra)."""
    graphs = build_graphs(c)
    sizes = [x.size(0) for x, _ in graphs]
    torch.manual_seed(c["seed"])
    om = OSCN(OM.SCN([c["H"]], c["act"], c["F"], c["K"]))
    big = max(range(len(graphs)), key=lambda i: sizes[i])
    ei = graphs[big][1]
    must = named_candidates(ei, sizes[big], c["graphs"][big][0])
    drops = [{"graphs": [(gx, e if i == big else gei) for i, (gx, gei) in enumerate(graphs)]}
             for (e,) in _drop_edges(ei, must=must)]
    draws = [{"graphs": relabel_graphs(graphs, s)} for s in YARDSTICK_SEEDS]
    maxima = (max(sizes), max(e.size(1) for _, e in graphs))
    chain_extra = len(sizes) * (max(sizes) + c["K"] + 4)      # the MinCUT contractions, as in test_scn_layered_routes
    return om, graphs, maxima, {"graphs": graphs}, drops, draws, chain_extra


def cotangent(graphs, K, g_mc=1.0, g_o=1.0):
    """d(g_mc mc + g_o o) on [S of every node (flat), mc, o]: S itself carries no gradient."""
    return torch.cat([torch.zeros(sum(x.size(0) for x, _ in graphs) * K), torch.tensor([g_mc, g_o])])


@functools.lru_cache(maxsize=None)
def _references_of(id):
    """The CPU references of a case under the cotangent (1, 1), computed once for every engine and test."""
    c = next(p.values[0] for p in CASES if p.values[0]["id"] == id)
    om, graphs, maxima, consts, drops, draws, chain_extra = build_case(c)
    ref = _references(what_of(c), om, {}, consts, cotangent(graphs, c["K"]), _scn_gates(c["act"]), ATOL, RTOL, drops,
                      1, chain_extra, draws)
    return om, graphs, maxima, ref


def supported(c, maxima):
    from graph_hscn import _hip
    lib = _hip.lib()
    args = (c["F"], c["H"], c["K"], *maxima)
    return int(lib.hscn_scn_resident_supported(*args)), int(lib.hscn_scn_resident_train_step_supported(*args))


# --------------------------------------------------------------------------- #
# the two engines
# --------------------------------------------------------------------------- #
class PPair(nn.Module):
    """``SCN.forward_graphs`` on the case's ``Batch`` (the oracle's argument is ignored: the batch is the same graphs)
    -> [S (flat), mc, o]."""

    def __init__(self, m):
        super().__init__()
        self.m, self.big = m, None

    def forward(self, graphs=None):
        S, mc, o = self.m.forward_graphs(self.big)
        return torch.cat([S.flatten(), mc.view(1), o.view(1)])


def _batch(graphs):
    from graph_hscn.data import Batch, Data
    return Batch.from_data_list([Data(x=x, edge_index=ei, num_nodes=x.size(0)) for x, ei in graphs]).to(DEV)


def _product(c, om, graphs):
    from graph_hscn.model.hscn import SCN
    pm = _load(PPair(SCN([c["H"]], c["act"], c["F"], c["K"])), om)
    pm.big = _batch(graphs)
    return pm


def _run_pair(pm, gy):
    pm.zero_grad(set_to_none=True)
    out = pm()
    assert pm.m.last_engine == "resident"
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    pm.big._scn_meta.check()
    return out.detach().clone(), {"p." + n: p.grad.detach().clone() for n, p in pm.named_parameters()}


def _run_step(pm, st):
    names = {id(p): n for n, p in pm.named_parameters()}
    st.run()
    torch.cuda.synchronize()
    st.check()
    out = torch.cat([st.S.flatten(), st.losses[:2]]).clone()
    return out, {"p." + names[id(p)]: g.detach().clone() for p, g in st.param_grads}


def _same(a, b):
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("c", CASES)
def test_stage_a_resident_against_the_float64_referee(c):
    from graph_hscn.step import ScnStructurePool, ScnTrainStep
    what = what_of(c)
    om, graphs, maxima, ref = _references_of(c["id"])
    fits = supported(c, maxima)
    print(f"[scn resident f64] {what}: (max_n, max_e) = {maxima} B = {len(graphs)} supported (pair, step) = {fits}")
    assert fits == (c["expect"]["pair"], c["expect"]["step"])
    pm = _product(c, om, graphs)
    gy = cotangent(graphs, c["K"])
    # ---- the launch pair under autograd
    pair = _run_pair(pm, gy)
    print(f"   worst ratio, launch pair: {_judge(what + ' pair', ref, *pair):.3f}")
    assert _same(_run_pair(pm, gy), pair), f"{what}: the launch pair does not repeat bit for bit"
    # ---- the one-launch step
    if not c["expect"]["step"]:
        with pytest.raises(RuntimeError):
            ScnTrainStep(pm.m, pm.big, one_launch=True)
        assert ScnTrainStep(pm.m, pm.big).one_launch is False
        return
    st = ScnTrainStep(pm.m, pm.big, one_launch=True)
    one = _run_step(pm, st)
    print(f"   worst ratio, one-launch step: {_judge(what + ' step', ref, *one):.3f}")
    assert torch.equal(one[0], pair[0]), f"{what}: the step's S and losses are not the pair's"
    assert _same(_run_step(pm, st), one), f"{what}: the one-launch step does not repeat bit for bit"
    # ---- the structure kept in HBM: built by the first run, loaded (cached front) by the second
    N, E = int(pm.big.num_nodes), int(pm.big.edge_index.size(1))
    cached = ScnTrainStep(pm.m, pm.big, one_launch=True, structure_pool=ScnStructurePool(torch.device(DEV), N, E, len(graphs)))
    first = _run_step(pm, cached)
    second = _run_step(pm, cached)
    assert _same(first, one), f"{what}: the step that exports its structure differs from the one that does not"
    assert _same(second, first), f"{what}: the step on the loaded structure differs from the one that built it"


@pytest.mark.parametrize("g_mc,g_o", [(0.5, 2.0), (0.0, 1.0)])
@pytest.mark.parametrize("id", ["A-row-tails-K4-F1", "E-K32-two-column-tiles"])
def test_pair_under_other_cotangents(id, g_mc, g_o):
    """The backward launch takes ``g_mc`` / ``g_o`` as device scalars and the step only ever sees ones: the pair under
    (0.5, 2.0) and (0, 1), each against oracle evaluations of its own (eight float32 draws, float64, dropped edges)."""
    c = next(p.values[0] for p in CASES if p.values[0]["id"] == id)
    om, graphs, maxima, consts, drops, draws, chain_extra = build_case(c)
    pm = _product(c, om, graphs)
    worst, _ = _check(f"{what_of(c)} pair g_mc={g_mc} g_o={g_o}", om, pm, {}, consts, cotangent(graphs, c["K"], g_mc, g_o),
                      gates=_scn_gates(c["act"]), drops=drops, chain_extra=chain_extra, draws=draws)
    assert pm.m.last_engine == "resident"
    pm.big._scn_meta.check()
    print(f"   worst ratio: {worst:.3f}")
