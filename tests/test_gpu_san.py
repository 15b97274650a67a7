"""SAN on the device: the attention over real and fake pairs and its two backward passes against tests/san_oracle.py
under the float64 referee (``referee_all`` / ``teeth`` of tests/helpers.py: the float32 and float64 restatements are the
two oracles, no constant of this file's own) at the tile, chunk and structure edges; the clamp; reproducibility; the
flag word; ``SANLayer`` and ``SAN`` at the three task levels; one ``train.train`` epoch.

Everything a case computes on the CPU sits in a function of its own (``_op_reference``, ``_structure_reference``,
``_clamp_reference``, ``_model_reference``): the seeds below were chosen by running those alone."""
import copy
import functools
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, LapPEConfig
from graph_hscn.data import Batch, Data, DataLoader
from graph_hscn.encoder.categorical import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
from graph_hscn.model.san import SAN
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.san import SANLayer
from graph_hscn.structure import Relation
from tests import san_oracle as SO
from tests.helpers import DEV, KinkGuard, grads_of, referee_all, teeth

pytestmark = pytest.mark.gpu

KEYS = ("out", "Z", "dq", "dk", "dv", "de", "dq2", "dk2e")
NAMES = ("q", "k", "v", "e", "q2", "k2e")


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------- #
# helpers: inputs, one oracle evaluation, one HIP evaluation
# --------------------------------------------------------------------------- #
def _inputs(N, E, heads, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    HC = heads * C
    x = {"q": torch.randn(N, HC, generator=g) * scale, "k": torch.randn(N, HC, generator=g) * scale,
         "v": torch.randn(N, HC, generator=g), "e": torch.randn(E, HC, generator=g) * 0.7 * scale,
         "q2": torch.randn(N, HC, generator=g) * scale, "k2e": torch.randn(N, HC, generator=g) * 0.7 * scale}
    return x, torch.randn(N, HC, generator=g)


def _oracle(x, ei, ptr, heads, gamma, full, go, dtype, skip=None):
    """One evaluation of the restatement in ``dtype``: every key of KEYS (dq2 / dk2e None without full_graph)."""
    t = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in x.items()}
    out, Z = SO.attention(t["q"], t["k"], t["v"], t["e"], t["q2"] if full else None, t["k2e"] if full else None, ei, ptr,
                          heads, gamma, full, skip)
    out.backward(go.to(dtype))
    return {"out": out.detach(), "Z": Z.detach(), "dq": t["q"].grad, "dk": t["k"].grad, "dv": t["v"].grad,
            "de": t["e"].grad, "dq2": t["q2"].grad if full else None, "dk2e": t["k2e"].grad if full else None}


def _hip_run(x, ei, ptr, heads, gamma, full, go, max_nodes=None, need=NAMES, check=True):
    N = x["q"].size(0)
    t = {k: v.detach().clone().to(DEV).requires_grad_(k in need) for k, v in x.items()}
    rel = Relation(ei.to(DEV), N, N)
    ptr32 = torch.tensor(ptr, dtype=torch.int32, device=DEV)
    if max_nodes is None:
        max_nodes = max(b - a for a, b in zip(ptr[:-1], ptr[1:]))
    out, Z = Fh.SANAttentionFn.apply(t["q"], t["k"], t["v"], t["e"], t["q2"] if full else None,
                                     t["k2e"] if full else None, rel, ptr32, max_nodes, heads, gamma, full)
    assert not Z.requires_grad
    out.backward(go.to(DEV))
    if check:
        rel.check()
        Fh.check_san(DEV)
    return {"out": out.detach(), "Z": Z.detach(), "dq": t["q"].grad, "dk": t["k"].grad, "dv": t["v"].grad,
            "de": t["e"].grad, "dq2": t["q2"].grad if full else None, "dk2e": t["k2e"].grad if full else None}


def _ptr(sizes):
    return [0] + np.cumsum(sizes).tolist()


def _random_batch(sizes, seed, per_node=2.0):
    """Graphs of ``sizes`` nodes with about ``per_node * n`` random directed edges each (loops and repeats as they
    fall), the whole edge list shuffled: a row's CSR slots are not its edge ids."""
    g = torch.Generator().manual_seed(seed)
    blocks, lo = [], 0
    for n in sizes:
        m = max(1, int(per_node * n)) if n > 1 else 0
        blocks.append(torch.randint(0, n, (2, m), generator=g) + lo)
        lo += n
    ei = torch.cat(blocks, 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous(), _ptr(sizes)


def _moved(bad64, o64):
    """{tensor: max|bad - full| / max|full|} of a float64 run with one term removed."""
    return {k: float((bad64[k] - v).abs().max()) / max(float(v.abs().max()), 1e-300) for k, v in o64.items()
            if v is not None and v.numel()}


def _material(bad64, o64):
    """The tensors a removed term moves by more than 1e-3 of their scale -- a thousand times the referee's float32
    tolerance, so the referee must reject each of them -- as the dict ``teeth`` takes."""
    return {k: bad64[k] for k, m in _moved(bad64, o64).items() if m > 1e-3}


def _best_drop(x, ei, ptr, heads, gamma, full, go, o64, candidates):
    """Of the candidate terms the one whose removal moves every tensor most (float64 runs): (skip, its gradients)."""
    best, best_score = None, -1.0
    for skip in candidates:
        d64 = _oracle(x, ei, ptr, heads, gamma, full, go, torch.float64, skip=skip)
        score = sorted(_moved(d64, o64).values())[2]            # the third-smallest: most tensors move materially
        if score > best_score:
            best, best_score = (skip, d64), score
    return best


# --------------------------------------------------------------------------- #
# 1. operator shapes: chunk and tile edges, a second tile
# --------------------------------------------------------------------------- #
OP_SIZES = (1, 2, 31, 32, 33, 64, 65, 97)
OP_WIDTHS = [(1, 4), (3, 12), (4, 8), (8, 64)]
OP_GAMMA = 0.1


def _fake_pairs(ei, ptr, g):
    """The ordered pairs (j, i) of graph g without a listed edge j -> i."""
    lo, hi = ptr[g], ptr[g + 1]
    listed = set(zip(ei[0].tolist(), ei[1].tolist()))
    return [(j, i) for i in range(lo, hi) for j in range(lo, hi) if (j, i) not in listed]


@functools.lru_cache(maxsize=None)
def _op_reference(heads, C, gamma=OP_GAMMA, full=True, with_teeth=True):
    ei, ptr = _random_batch(OP_SIZES, seed=3)
    N, E = ptr[-1], ei.size(1)
    x, go = _inputs(N, E, heads, C, seed=100 + heads * 1000 + C)
    o32 = _oracle(x, ei, ptr, heads, gamma, full, go, torch.float32)
    o64 = _oracle(x, ei, ptr, heads, gamma, full, go, torch.float64)
    drops = {}
    if with_teeth:
        # a real edge and a fake pair of the two-node graph and of the 31-node graph: whichever moves the most tensors
        in_g = lambda e, g: ptr[g] <= int(ei[1, e]) < ptr[g + 1]
        real = [("real", e) for g in (1, 2) for e in [e for e in range(E) if in_g(e, g)][:2]]
        drops["real"] = _best_drop(x, ei, ptr, heads, gamma, full, go, o64, real)
        if full:
            fake = [("fake", p) for g in (1, 2) for p in _fake_pairs(ei, ptr, g)[:2]]
            drops["fake"] = _best_drop(x, ei, ptr, heads, gamma, full, go, o64, fake)
    return x, go, ei, ptr, o32, o64, drops


@pytest.mark.parametrize("heads,C", OP_WIDTHS)
def test_operator_at_the_chunk_and_tile_edges_under_the_float64_referee(heads, C):
    what = f"SAN attention H={heads} C={C}"
    x, go, ei, ptr, o32, o64, drops = _op_reference(heads, C)
    deg = torch.bincount(ei[1], minlength=ptr[-1])
    assert int(deg.max()) >= 2 and int((deg == 0).sum()) >= 1          # rows with several real pairs, rows with none
    got = _hip_run(x, ei, ptr, heads, OP_GAMMA, True, go)
    assert got["Z"].shape == (ptr[-1], heads) and not bool(torch.isnan(got["out"]).any())
    referee_all(got, o32, o64, what)
    for g in range(len(OP_SIZES)):                                        # and every graph by itself
        rows = slice(ptr[g], ptr[g + 1])
        sub = lambda d: {k: d[k][rows] for k in KEYS if k != "de"}
        referee_all(sub(got), sub(o32), sub(o64), f"{what}, graph of {OP_SIZES[g]}")
    for kind, core in (("real", {"out", "Z", "dq", "dk", "dv", "de"}), ("fake", {"out", "Z", "dq2", "dk2e", "dv"})):
        skip, d64 = drops[kind]
        reached = _material(d64, o64)
        assert core <= set(reached), (kind, skip, sorted(reached))
        teeth(got, o32, o64, reached, f"{what} [{kind} term {skip[1]} dropped]")


@pytest.mark.parametrize("gamma,full", [(0.0, True), (4.0, True), (0.1, False)])
def test_gamma_and_full_graph_off_on_the_same_batch(gamma, full):
    heads, C = 3, 12
    what = f"SAN attention gamma={gamma} full_graph={full}"
    x, go, ei, ptr, o32, o64, drops = _op_reference(heads, C, gamma, full, with_teeth=gamma != 0.0)
    got = _hip_run(x, ei, ptr, heads, gamma, full, go)
    referee_all(got, o32, o64, what)
    if not full:
        assert got["dq2"] is None and got["dk2e"] is None
        empty = (torch.bincount(ei[1], minlength=ptr[-1]) == 0).nonzero().flatten().tolist()
        assert empty and not got["out"][empty].any() and not got["Z"][empty].any()       # no in-edge: zeros
        plain = _op_reference(heads, C, 0.0, True, with_teeth=False)[5]                   # gamma = 0 is the same thing
        assert torch.equal(plain["out"], o64["out"]) and torch.equal(plain["Z"], o64["Z"])
    if gamma == 0.0:                                                                       # b = 0: nothing reaches q2 / k2e
        assert not got["dq2"].any() and not got["dk2e"].any()
    for kind, (skip, d64) in drops.items():
        teeth(got, o32, o64, _material(d64, o64), f"{what} [{kind} term {skip[1]} dropped]")


# --------------------------------------------------------------------------- #
# 2. structure cases, each one small graph inside a batch
# --------------------------------------------------------------------------- #
ST_HEADS, ST_C, ST_GAMMA = 2, 8, 0.5
ST_CASES = ("no edges", "one directed edge", "a self-loop", "a duplicated edge", "complete with self-loops",
            "an isolated node", "in-degree above 64")
ST_HUB_N, ST_HUB_DEG = 70, 80


def _structure_graphs():
    g = torch.Generator().manual_seed(11)
    n_c = 4
    complete = torch.tensor([[j for j in range(n_c) for i in range(n_c)], [i for j in range(n_c) for i in range(n_c)]])
    hub_src = torch.cat([torch.arange(1, ST_HUB_N), torch.randint(1, ST_HUB_N, (ST_HUB_DEG - ST_HUB_N + 1,), generator=g)])
    hub = torch.cat([torch.stack([hub_src, torch.zeros_like(hub_src)]), torch.randint(0, ST_HUB_N, (2, 40), generator=g)], 1)
    return [("filler", 5, torch.randint(0, 5, (2, 9), generator=g)),
            ("no edges", 4, torch.zeros(2, 0, dtype=torch.long)),
            ("one directed edge", 3, torch.tensor([[2], [0]])),
            ("a self-loop", 3, torch.tensor([[1, 0], [1, 2]])),
            ("a duplicated edge", 3, torch.tensor([[0, 2, 0], [1, 0, 1]])),
            ("complete with self-loops", n_c, complete),
            ("an isolated node", 5, torch.tensor([[0, 1, 2, 0], [1, 2, 0, 2]])),          # nodes 3, 4 touch no edge
            ("in-degree above 64", ST_HUB_N, hub),
            ("filler", 6, torch.randint(0, 6, (2, 11), generator=g))]


@functools.lru_cache(maxsize=None)
def _structure_reference():
    graphs = _structure_graphs()
    ptr = _ptr([n for _, n, _ in graphs])
    ei = torch.cat([e + ptr[g] for g, (_, _, e) in enumerate(graphs)], 1)
    first_edge = dict(zip([name for name, _, _ in graphs], np.cumsum([0] + [e.size(1) for _, _, e in graphs]).tolist()))
    perm = torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(12))
    where = torch.empty_like(perm)
    where[perm] = torch.arange(perm.numel())                              # edge k of the unshuffled list is edge where[k]
    ei = ei[:, perm].contiguous()
    x, go = _inputs(ptr[-1], ei.size(1), ST_HEADS, ST_C, seed=13)
    o32 = _oracle(x, ei, ptr, ST_HEADS, ST_GAMMA, True, go, torch.float32)
    o64 = _oracle(x, ei, ptr, ST_HEADS, ST_GAMMA, True, go, torch.float64)
    lo = {name: ptr[g] for g, (name, _, _) in enumerate(graphs)}
    edge = lambda name, k: int(where[first_edge[name] + k])
    skips = {"no edges": ("fake", (lo["no edges"] + 1, lo["no edges"] + 1)),                     # the diagonal counts
             "one directed edge": ("fake", (lo["one directed edge"], lo["one directed edge"] + 2)),  # the reverse pair is fake
             "a self-loop": ("real", edge("a self-loop", 0)),
             "a duplicated edge": ("real", max(edge("a duplicated edge", 0), edge("a duplicated edge", 2))),
             "complete with self-loops": ("real", edge("complete with self-loops", 5)),
             "an isolated node": ("fake", (lo["an isolated node"] + 3, lo["an isolated node"] + 4)),
             "in-degree above 64": ("real", edge("in-degree above 64", 68))}
    drops = {name: _oracle(x, ei, ptr, ST_HEADS, ST_GAMMA, True, go, torch.float64, skip=s) for name, s in skips.items()}
    return x, go, ei, ptr, o32, o64, drops, {name: g for g, (name, _, _) in enumerate(graphs)}


_ST_GOT = {}


def _structure_got():
    if not _ST_GOT:
        x, go, ei, ptr = _structure_reference()[:4]
        _ST_GOT["got"] = _hip_run(x, ei, ptr, ST_HEADS, ST_GAMMA, True, go)
        moved = dict(x, q2=x["q2"] * 1.5 + 0.25, k2e=x["k2e"] - 0.5)    # other fake projections, everything else the same
        _ST_GOT["moved"] = _hip_run(moved, ei, ptr, ST_HEADS, ST_GAMMA, True, go)
    return _ST_GOT["got"], _ST_GOT["moved"]


@pytest.mark.parametrize("case", ST_CASES)
def test_structure_cases_under_the_float64_referee(case):
    x, go, ei, ptr, o32, o64, drops, index = _structure_reference()
    got, moved = _structure_got()
    g = index[case]
    rows = slice(ptr[g], ptr[g + 1])
    mine = ((ei[1] >= ptr[g]) & (ei[1] < ptr[g + 1])).nonzero().flatten()
    sub = lambda d: {k: (d[k][mine] if k == "de" else d[k][rows]) for k in KEYS}
    what = f"SAN attention, {case}"
    referee_all(got, o32, o64, "SAN attention, the structure batch")
    referee_all(sub(got), sub(o32), sub(o64), what)
    reached = {k: v for k, v in _material(sub(drops[case]), sub(o64)).items() if v.numel()}
    assert {"out", "Z"} <= set(reached), sorted(reached)
    teeth(sub(got), sub(o32), sub(o64), reached, what)
    if case == "no edges":
        assert mine.numel() == 0 and bool((got["Z"][rows] > 0).all())
        assert not got["dq"][rows].any() and not got["dk"][rows].any()                   # no real pair reaches q or k
    if case == "complete with self-loops":                                              # Z_fake = 0: q2 / k2e do not enter
        for k in ("out", "Z", "dq", "dk", "dv"):
            assert np.array_equal(_bits(got[k][rows]), _bits(moved[k][rows])), k
        assert np.array_equal(_bits(got["de"][mine]), _bits(moved["de"][mine]))
        assert not got["dq2"][rows].any() and not got["dk2e"][rows].any()
        assert not np.array_equal(_bits(got["out"]), _bits(moved["out"]))                # (they do enter elsewhere)
    if case == "an isolated node":
        alone = slice(ptr[g] + 3, ptr[g] + 5)
        assert not got["dq"][alone].any() and not got["dk"][alone].any() and bool(got["dq2"][alone].any())
    if case == "in-degree above 64":
        assert int(torch.bincount(ei[1], minlength=ptr[-1])[ptr[g]]) >= ST_HUB_DEG > 64      # (the 40 further edges may add)


# --------------------------------------------------------------------------- #
# 3. the clamp
# --------------------------------------------------------------------------- #
CLAMP_HEADS, CLAMP_C, CLAMP_SEED, CLAMP_GAMMA = 4, 4, 0, 1.0
CLAMP_SIZES = (5, 33, 12)


@functools.lru_cache(maxsize=None)
def _clamp_reference(seed):
    """A small batch with q, k, e, q2, k2e x 2.5: float64 scores of both kinds saturate on both sides.  Returns the inputs,
    the float64 scores and how far float32 can be from them (the seed search reads the last two alone)."""
    ei, ptr = _random_batch(CLAMP_SIZES, seed=21, per_node=3.0)
    x, go = _inputs(ptr[-1], ei.size(1), CLAMP_HEADS, CLAMP_C, seed=seed, scale=2.5)
    x64 = {k: v.double() for k, v in x.items()}
    _, _, s_real, s_fake = SO.attention(x64["q"], x64["k"], x64["v"], x64["e"], x64["q2"], x64["k2e"], ei, ptr,
                                        CLAMP_HEADS, CLAMP_GAMMA, True, want_scores=True)
    xa = {k: v.abs() for k, v in x64.items()}
    _, _, m_real, m_fake = SO.attention(xa["q"], xa["k"], xa["v"], xa["e"], xa["q2"], xa["k2e"], ei, ptr, CLAMP_HEADS,
                                        CLAMP_GAMMA, True, want_scores=True)
    # a float32 score of C products and C adds: within (C + 2) 2^-24 of sum |terms| / sqrt(C)
    bound = (CLAMP_C + 2) * 2.0 ** -24 * max(float(m_real.max()), float(m_fake.max()))
    return x, go, ei, ptr, s_real, s_fake, bound


def test_clamp_gates_the_gradients_on_both_sides():
    x, go, ei, ptr, s_real, s_fake, bound = _clamp_reference(CLAMP_SEED)
    for s in (s_real, s_fake):                              # asserted on the CPU before the device is touched
        n = s.numel()
        assert int((s > 5).sum()) >= 0.03 * n and int((s < -5).sum()) >= 0.03 * n
        assert int((s.abs() < 5).sum()) >= 0.20 * n
        assert float((s.abs() - 5).abs().min()) > 1e-3      # no score near a bound ...
    assert bound < 1e-4                                     # ... and float32 is this close: both take the same side
    got = _hip_run(x, ei, ptr, CLAMP_HEADS, CLAMP_GAMMA, True, go)
    o32 = _oracle(x, ei, ptr, CLAMP_HEADS, CLAMP_GAMMA, True, go, torch.float32)
    o64 = _oracle(x, ei, ptr, CLAMP_HEADS, CLAMP_GAMMA, True, go, torch.float64)
    referee_all(got, o32, o64, "clamped SAN attention")
    # an edge's feature gradient is zero exactly where its score is saturated (s_real: targets ascending, then sources
    # ascending, then list order -- the restatement's order)
    order = []
    for i, row in SO.pairs(ei, ptr):
        order += [e for _, ids in row for e in ids]
    saturated = torch.zeros(ei.size(1), CLAMP_HEADS, dtype=torch.bool)
    saturated[order] = s_real.abs() > 5
    de = got["de"].view(-1, CLAMP_HEADS, CLAMP_C).cpu()
    assert bool(saturated.any()) and not de[saturated].any() and bool(de[~saturated].any())
    assert not o64["de"].view(-1, CLAMP_HEADS, CLAMP_C)[saturated].any()


# --------------------------------------------------------------------------- #
# 4. bits
# --------------------------------------------------------------------------- #
def _two_graphs(seed=31):
    ei_a, _ = _random_batch((33,), seed)
    ei_b, _ = _random_batch((12,), seed + 1)
    xa, ga = _inputs(33, ei_a.size(1), 4, 8, seed + 2)
    xb, gb = _inputs(12, ei_b.size(1), 4, 8, seed + 3)
    return (ei_a, xa, ga), (ei_b, xb, gb)


def _cat(first, second):
    (e1, x1, g1), (e2, x2, g2) = first, second
    n1 = x1["q"].size(0)
    return (torch.cat([e1, e2 + n1], 1), {k: torch.cat([x1[k], x2[k]]) for k in x1}, torch.cat([g1, g2]),
            [0, n1, n1 + x2["q"].size(0)])


def test_two_runs_give_the_same_bits_and_a_graph_has_them_wherever_it_stands():
    A, B = _two_graphs()
    ei, x, go, ptr = _cat(A, B)
    first = _hip_run(x, ei, ptr, 4, 0.1, True, go)
    again = _hip_run(x, ei, ptr, 4, 0.1, True, go)
    for k in KEYS:
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
    alone = _hip_run(A[1], A[0], [0, 33], 4, 0.1, True, A[2])
    ei2, x2, go2, ptr2 = _cat(B, A)
    last = _hip_run(x2, ei2, ptr2, 4, 0.1, True, go2)
    EA = A[0].size(1)
    for k in KEYS:
        a = alone[k]
        f = first[k][:EA] if k == "de" else first[k][:33]
        l = last[k][-EA:] if k == "de" else last[k][-33:]
        assert np.array_equal(_bits(a), _bits(f)), (k, "first in the batch")
        assert np.array_equal(_bits(a), _bits(l)), (k, "last in the batch")


def test_only_what_needs_a_gradient_is_computed():
    A, B = _two_graphs()
    ei, x, go, ptr = _cat(A, B)
    full = _hip_run(x, ei, ptr, 4, 0.1, True, go)
    key = {"q": "dq", "k": "dk", "v": "dv", "e": "de", "q2": "dq2", "k2e": "dk2e"}
    for only in NAMES:
        got = _hip_run(x, ei, ptr, 4, 0.1, True, go, need=(only,))
        assert np.array_equal(_bits(got[key[only]]), _bits(full[key[only]])), only
        assert all(got[key[n]] is None for n in NAMES if n != only), only
    t = {k: v.to(DEV) for k, v in x.items()}                     # nothing needs one: no graph is recorded
    out, _ = Fh.SANAttentionFn.apply(t["q"], t["k"], t["v"], t["e"], t["q2"], t["k2e"], Relation(ei.to(DEV), 45, 45),
                                     torch.tensor(ptr, dtype=torch.int32, device=DEV), 33, 4, 0.1, True)
    assert not out.requires_grad and np.array_equal(_bits(out), _bits(full["out"]))


# --------------------------------------------------------------------------- #
# 5. the flag word
# --------------------------------------------------------------------------- #
def test_an_edge_into_another_graph_is_skipped_counted_as_fake_and_flagged():
    # graphs of 4 and 5 nodes; the last listed edge leaves node 6 (second graph) for node 1 (first graph)
    ei = torch.tensor([[0, 1, 2, 3, 4, 5, 7, 8, 6], [1, 2, 0, 0, 5, 6, 4, 7, 1]])
    ptr = [0, 4, 9]
    x, go = _inputs(9, 9, 2, 8, seed=41)
    o32 = _oracle(x, ei, ptr, 2, 0.5, True, go, torch.float32)    # the restatement takes edges inside a graph only
    o64 = _oracle(x, ei, ptr, 2, 0.5, True, go, torch.float64)
    assert not o64["de"][8].any()
    got = _hip_run(x, ei, ptr, 2, 0.5, True, go, check=False)
    referee_all(got, o32, o64, "SAN attention with an edge between two graphs")
    assert not got["de"][8].any()
    with pytest.raises(ValueError, match="outside its target's graph"):
        Fh.check_san(DEV)
    Fh.check_san(DEV)                                             # read and cleared


def test_a_graph_beyond_max_nodes_gets_nan_rows_and_its_flag():
    ei, ptr = _random_batch((3, 9, 4), seed=43)
    x, go = _inputs(16, ei.size(1), 2, 8, seed=44)
    good = _hip_run(x, ei, ptr, 2, 0.1, True, go)
    got = _hip_run(x, ei, ptr, 2, 0.1, True, go, max_nodes=8, check=False)
    big = slice(3, 12)
    for k in ("out", "Z", "dq", "dk", "dv", "dq2", "dk2e"):
        assert bool(torch.isnan(got[k][big]).all()), k
        for rows in (slice(0, 3), slice(12, 16)):                 # the other graphs are what they always are
            assert np.array_equal(_bits(got[k][rows]), _bits(good[k][rows])), k
    with pytest.raises(ValueError, match="more nodes than the batch's max_nodes"):
        Fh.check_san(DEV)
    Fh.check_san(DEV)


# --------------------------------------------------------------------------- #
# 6. the layer and the model
# --------------------------------------------------------------------------- #
M_F, M_D, M_C, M_L, M_HEADS, M_DE, M_GAMMA = 6, 16, 8, 2, 4, 3, 0.5     # (the pair decoder takes widths 4 k)
M_SIZES = (5, 9, 1, 7, 6)
M_PE, M_K = 4, 4
M_CASES = [(lvl, enc) for lvl in ("graph", "node", "link") for enc in ("categorical+lappe", "linear")]
# (task level, encoders) -> seed: the first of the seeds 0, 1, ... whose float64 run meets the gate condition
# (``_gate_margin`` > 1.5: every ReLU input farther from zero than 6 x the referee's limit for its tensor).  A CPU-only
# choice: ``_model_reference`` runs no product code.
M_SEEDS = {case: 0 for case in M_CASES}
LAYER_SEED = 0


def _model_batch(seed, enc, level):
    g = torch.Generator().manual_seed(700 + seed)
    graphs = []
    for n in M_SIZES:
        half = torch.randint(0, n, (2, n + 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        E = ei.size(1)
        if enc == "linear":
            d = Data(x=torch.randn(n, M_F, generator=g), edge_index=ei, y=torch.zeros(1, M_C))
            d.edge_attr = torch.randn(E, M_DE, generator=g)
        else:
            xs = torch.stack([torch.randint(0, c, (n,), generator=g) for c in ATOM_FEATURE_DIMS], 1)
            d = Data(x=xs, edge_index=ei, y=torch.zeros(1, M_C))
            d.edge_attr = torch.stack([torch.randint(0, c, (E,), generator=g) for c in BOND_FEATURE_DIMS], 1)
            vec = torch.randn(n, M_K, generator=g)
            val = torch.rand(n, M_K, generator=g) * 2.0
            vec[:, min(n, M_K):] = float("nan")
            val[:, min(n, M_K):] = float("nan")
            d.eigvecs_sn, d.eigvals_sn = vec, val.unsqueeze(2)
        if level == "link":
            pairs = torch.randperm(n * n, generator=g)[:min(6, n * n)]
            d.edge_label_index = torch.stack([pairs // n, pairs % n])
            d.edge_label = torch.randint(0, 2, (pairs.numel(),), generator=g).float()
        graphs.append(d)
    return Batch.from_data_list(graphs)


def _model_run(ref, b, gy, dtype, skip=None):
    m = copy.deepcopy(ref).to(dtype)
    seen = {}
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    floats = b.x.is_floating_point()
    stats = (b.eigvecs_sn.to(dtype), b.eigvals_sn.to(dtype)) if hasattr(m, "pe_encoder") else None
    out = m(b.x.to(dtype) if floats else b.x, b.edge_index, b.edge_attr.to(dtype) if floats else b.edge_attr, b.batch,
            b.ptr.tolist(), b.edge_label_index if m.task_level == "link" else None, stats, skip)
    out.backward(gy.to(dtype))
    grads = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    return grads, out.detach(), seen


@functools.lru_cache(maxsize=None)
def _model_reference(level, enc, seed):
    b = _model_batch(seed, enc, level)
    torch.manual_seed(seed)
    if enc == "linear":
        ref = SO.SANRef(M_F, M_D, M_C, M_L, M_HEADS, M_GAMMA, True, level, edge_dim=M_DE)
    else:
        ref = SO.SANRef(M_F, M_D, M_C, M_L, M_HEADS, M_GAMMA, True, level, node_encoder=ATOM_FEATURE_DIMS,
                        edge_encoder=BOND_FEATURE_DIMS, lappe=(M_PE, 2, 1))
    rows = {"graph": (len(M_SIZES), M_C), "node": (sum(M_SIZES), M_C)}.get(level) or (int(b.edge_label_index.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))
    r32 = _model_run(ref, b, gy, torch.float32)
    r64 = _model_run(ref, b, gy, torch.float64)
    last = int(b.edge_index.size(1)) - 1
    d_real = _model_run(ref, b, gy, torch.float64, skip=("real", last))                  # the last listed edge
    lo = int(b.ptr[1])                                                                    # the second graph
    fake = _fake_pairs(b.edge_index, b.ptr.tolist(), 1)[0]
    d_fake = _model_run(ref, b, gy, torch.float64, skip=("fake", fake))
    assert lo <= fake[0] < int(b.ptr[2])
    return ref, b, gy, r32, r64, d_real, d_fake


def _gate_margin(g32, g64):
    """min over the ReLU inputs of |value| / (4 x the referee's limit of its tensor): > 1 meets the gate condition."""
    worst = float("inf")
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        worst = min(worst, float(v64.abs().min()) / (4.0 * bound))
    return worst


def _check_gates(g32, g64, what):
    assert set(g32) == set(g64) and g64
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"{what} {tag}")


def _product_model(level, enc):
    if enc == "linear":
        return SAN(M_F, M_D, M_C, M_L, M_HEADS, ACT_DICT["relu"], 0.0, "layer", level, gamma=M_GAMMA).to(DEV)
    pe = LapPEConfig(dim_in=9, dim_emb=M_D, dim_pe=M_PE, layers=2, post_layers=1, eigen_max_freqs=M_K, sign_flip=False)
    return SAN(9, M_D, M_C, M_L, M_HEADS, ACT_DICT["relu"], 0.0, "layer", level, "atom", "bond", M_GAMMA,
               pos_enc=pe).to(DEV)


@pytest.mark.parametrize("level,enc", M_CASES)
def test_san_model_under_the_float64_referee(level, enc):
    from graph_hscn.train import batching
    what = f"SAN {level} level, {enc} encoders"
    ref, b, gy, (o32, y32, g32), (o64, y64, g64), (dr64, dry64, _), (df64, dfy64, _) = \
        _model_reference(level, enc, M_SEEDS[(level, enc)])
    assert len(g64) == M_L + 1 + (3 if enc != "linear" else 0)
    _check_gates(g32, g64, what)
    pm = _product_model(level, enc)
    bd = batching.to_device(pm, b, DEV)
    if enc == "linear":
        pm.edge_encoder.materialize(M_DE, bd.edge_attr)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    back = copy.deepcopy(ref)                               # and the other way round
    back.load_state_dict({k: v.detach().cpu().clone() for k, v in pm.state_dict().items()}, strict=True)
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in ref.state_dict().items())
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    pm.check_flags()
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dry64}, what + " [a real edge dropped]")
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dfy64}, what + " [a fake pair dropped]")
    got = {k: v for k, v in grads_of(pm).items() if k in o64}
    assert set(got) == set(o64)
    referee_all(got, o32, o64, what)
    reached = _material(dr64, o64)
    assert {"p.node_encoder.weight", "p.edge_encoder.weight", "p.layers.0.attention.Q.weight",
            "p.layers.0.attention.E.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what + " [a real edge dropped]")
    reached = _material(df64, o64)
    assert {"p.fake_edge_emb.weight", "p.layers.0.attention.Q_2.weight", "p.layers.0.attention.K_2.weight",
            "p.layers.0.attention.E_2.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what + " [a fake pair dropped]")


@functools.lru_cache(maxsize=None)
def _layer_reference(seed):
    b = _model_batch(seed, "linear", "node")
    g = torch.Generator().manual_seed(900 + seed)
    N, E = b.num_nodes, int(b.edge_index.size(1))
    x = {"x": torch.randn(N, M_D, generator=g), "edge_attr": torch.randn(E, M_D, generator=g),
         "fake": torch.randn(1, M_D, generator=g)}
    gy = torch.randn(N, M_D, generator=g)
    torch.manual_seed(seed)
    ref = SO.SANLayerRef(M_D, M_HEADS, M_GAMMA, True)

    def run(dtype, skip=None):
        m = copy.deepcopy(ref).to(dtype)
        seen = {}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        t = {k: v.clone().to(dtype).requires_grad_(True) for k, v in x.items()}
        out = m(t["x"], b.edge_index, t["edge_attr"], b.ptr.tolist(), t["fake"], skip)
        out.backward(gy.to(dtype))
        grads = {"x." + k: v.grad for k, v in t.items()}
        grads.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
        grads["out"] = out.detach()
        return grads, seen

    return ref, b, x, gy, run(torch.float32), run(torch.float64), run(torch.float64, ("real", E - 1))[0]


def test_san_layer_under_the_float64_referee():
    what = "SANLayer"
    ref, b, x, gy, (o32, g32), (o64, g64), d64 = _layer_reference(LAYER_SEED)
    _check_gates(g32, g64, what)
    layer = SANLayer(M_D, M_HEADS, M_GAMMA, True).to(DEV)
    layer.load_state_dict(ref.state_dict(), strict=True)
    t = {k: v.clone().to(DEV).requires_grad_(True) for k, v in x.items()}
    bd = b.to(DEV)
    out = layer(t["x"], bd.edge_index, t["edge_attr"], bd, t["fake"])
    out.backward(gy.to(DEV))
    Fh.check_san(DEV)
    got = grads_of(layer, **t)
    got["out"] = out.detach()
    referee_all(got, o32, o64, what)
    reached = _material(d64, o64)
    assert {"out", "x.x", "x.edge_attr", "p.attention.Q.weight", "p.attention.E.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what)


# --------------------------------------------------------------------------- #
# 7. training, and the entry points that do not take the model
# --------------------------------------------------------------------------- #
def _peptides(count=8):
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    rng, edge_rng = np.random.default_rng(5), np.random.default_rng(6)
    return [make_graph(rng, SHAPES["peptides_func"], n=n, edge_features=True, edge_rng=edge_rng)
            for n in (1, 2, 7, 40, 23, 12, 31, 5)[:count]]


def test_one_epoch_of_train_runs_with_a_finite_loss_and_clean_flags():
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.train.train import train
    torch.manual_seed(3)
    pe = RWSEConfig(dim_in=9, dim_emb=16, dim_pe=4, ksteps=8)
    m = SAN(9, 16, 10, 2, 4, ACT_DICT["relu"], 0.1, "layer", "graph", "atom", "bond", 0.1, pos_enc=pe).to(DEV)
    m.dropout_seed = 5
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    graphs = _peptides()
    cfg = SimpleNamespace(model_type="san", epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10,
                          min_delta=0.0, metric="ap")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    history = train(None, opt, cfg, [DataLoader(graphs, 4), DataLoader(graphs, 8)], m)
    torch.cuda.synchronize()
    assert len(history) == 1 and np.isfinite(history[0][0])
    m.check_flags()
    for k in ("fake_edge_emb.weight", "layers.0.attention.Q_2.weight", "layers.1.attention.E.weight", "edge_encoder.weight"):
        assert not torch.equal(before[k], m.state_dict()[k]), k                # the step reached them


def test_the_captured_step_refuses_the_model_with_its_own_reason():
    from graph_hscn.replay import CapturedStep
    from graph_hscn.train import batching
    m = SAN(9, 16, 10, 1, 4, ACT_DICT["relu"], node_encoder="atom", edge_encoder="bond").to(DEV)
    bd = batching.to_device(m, Batch.from_data_list(_peptides(4)), DEV)
    with pytest.raises(RuntimeError, match=re.escape(m.resident_reason())):
        CapturedStep(m, SimpleNamespace(batch=bd), "cross_entropy")
    m.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="SAN's attention over real and fake edges"):
        m(bd)
