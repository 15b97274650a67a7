"""Exphormer on the device: the expander kernel against its numpy restatement bit for bit; the typed sparse attention,
its three backward passes and the table gradient against tests/exphormer_oracle.py under the float64 referee
(``referee_all`` / ``teeth`` of tests/helpers.py: the float32 and float64 restatements are the two oracles, no constant
of this file's own); long rows, the clamp, reproducibility; ``GPS(global_model="exphormer")`` at the three task levels.

Everything a case computes on the CPU sits in a function of its own (``_op_reference``, ``_clamp_reference``,
``_model_reference``): the seeds below were chosen by running those alone."""
import copy
import math

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import Batch, Data
from graph_hscn.model.gps import GPS
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import ExphormerStructure
from tests import exphormer_oracle as XO
from tests.helpers import DEV, KinkGuard, grads_of, referee_all, teeth

pytestmark = pytest.mark.gpu

KEYS = ("out", "dq", "dk", "dv", "de_edge", "de_type")


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------- #
# 1. the expander kernel
# --------------------------------------------------------------------------- #
def _expander(sizes, d, seed, graph_ids=None, max_nodes=None):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.tensor(sizes), 0).to(torch.int32)
    gids = None if graph_ids is None else torch.tensor(graph_ids, dtype=torch.int64, device=DEV)
    out = Fh.expander_edges(ptr.to(DEV), d, seed, gids, max_nodes=max(sizes) if max_nodes is None else max_nodes,
                            num_nodes=int(sum(sizes)))
    return out.cpu()


@pytest.mark.parametrize("d", [2, 6, 32])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257, 2048])
def test_expander_kernel_equals_the_restatement(n, d):
    got = _expander([n], d, seed=0x123456789)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, n * d)
    assert torch.equal(got, XO.expander_edges([n], d, 0x123456789))
    Fh.check_expander(DEV)


def test_expander_kernel_on_a_mixed_batch_with_graph_ids():
    sizes = [5, 1, 64, 2, 300, 65, 3, 0, 17]
    assert torch.equal(_expander(sizes, 6, seed=7), XO.expander_edges(sizes, 6, 7))
    gids = [40, 3, 2 ** 31 - 1, 0, 5, 5, 77, 1, 9]
    got = _expander(sizes, 4, seed=2 ** 40 + 3, graph_ids=gids)
    assert torch.equal(got, XO.expander_edges(sizes, 4, 2 ** 40 + 3, gids))
    # a graph's edges follow its id, not its place
    alone = _expander([300], 4, seed=2 ** 40 + 3, graph_ids=[5])
    lo = sum(sizes[:4])
    assert torch.equal(got[:, 4 * lo:4 * (lo + 300)] - lo, alone)
    Fh.check_expander(DEV)


def test_a_graph_beyond_the_envelope_is_flagged_and_the_others_are_exact():
    sizes = [6, 2049, 9]
    got = _expander(sizes, 2, seed=1, max_nodes=2048)
    ref = XO.expander_edges(sizes, 2, 1)
    assert torch.equal(got[:, :12], ref[:, :12]) and torch.equal(got[:, 2 * 2055:], ref[:, 2 * 2055:])
    assert bool((got[:, 12:2 * 2055] == -1).all())
    with pytest.raises(ValueError, match="more nodes than max_nodes"):
        Fh.check_expander(DEV)
    Fh.check_expander(DEV)                      # read and cleared


# --------------------------------------------------------------------------- #
# 2. the operator on a multigraph
# --------------------------------------------------------------------------- #
def _oracle(x, ei, erow, El, heads, go, dtype, skip=None, swap=None):
    """One evaluation of the restatement in ``dtype``: {out, dq, dk, dv, de_edge, de_type} (de_edge None without rows)."""
    t = {k: (None if v is None else v.detach().clone().to(dtype).requires_grad_(True)) for k, v in x.items()}
    out = XO.attention(t["q"], t["k"], t["v"], t["e_edge"], t["e_type"], ei, erow, El, heads, skip=skip, swap=swap)
    out.backward(go.to(dtype))
    return {"out": out.detach(), "dq": t["q"].grad, "dk": t["k"].grad, "dv": t["v"].grad,
            "de_edge": None if t["e_edge"] is None else t["e_edge"].grad, "de_type": t["e_type"].grad}


def _hip_run(x, struct, heads, go, q_offset=False):
    t = {k: (None if v is None else v.detach().clone().to(DEV).requires_grad_(True)) for k, v in x.items()}
    q = t["q"]
    if q_offset:                                # q at a 4-byte offset: every pass takes the VEC = 1 path
        flat = torch.zeros(q.numel() + 1, device=DEV)
        flat[1:] = x["q"].to(DEV).flatten()
        q = flat[1:].view_as(x["q"]).requires_grad_(True)
        assert q.data_ptr() % 16 == 4 and q.is_contiguous()
    out = Fh.ExphormerAttentionFn.apply(q, t["k"], t["v"], t["e_edge"], t["e_type"], struct, heads)
    out.backward(go.to(DEV))
    struct.rel.check()
    return {"out": out.detach(), "dq": q.grad, "dk": t["k"].grad, "dv": t["v"].grad,
            "de_edge": None if t["e_edge"] is None else t["e_edge"].grad, "de_type": t["e_type"].grad}


def _inputs(rows, El, T, heads, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    HC = heads * C
    x = {"q": torch.randn(rows, HC, generator=g) * scale, "k": torch.randn(rows, HC, generator=g) * scale,
         "v": torch.randn(rows, HC, generator=g) * scale,
         "e_edge": torch.randn(El, HC, generator=g) * 0.5 * scale if El else None,
         "e_type": torch.randn(T, HC, generator=g) * 0.5 * scale}
    return x, torch.randn(rows, HC, generator=g)


OP_N, OP_E, OP_NV = 37, 150, 1
OP_ISOLATED = (3, 11, 20, 36)


def _op_graph(with_edge_rows):
    """37 rows, 150 union edges in random order: four isolated rows, two self loops, one edge three times; 90 edges
    with a feature row of their own (a permutation, so erow[slot] != slot), the rest over all T = 4 types."""
    g = torch.Generator().manual_seed(5)
    live = torch.tensor([i for i in range(OP_N) if i not in OP_ISOLATED])
    ei = live[torch.randint(0, live.numel(), (2, OP_E), generator=g)]
    ei[:, 0] = torch.tensor([7, 7])
    ei[:, 1] = torch.tensor([30, 30])
    ei[:, 2] = ei[:, 3] = ei[:, 4] = torch.tensor([5, 9])
    ei = ei[:, torch.randperm(OP_E, generator=g)].contiguous()
    T = 2 + 2 * OP_NV
    El = 90 if with_edge_rows else 0
    erow = torch.empty(OP_E, dtype=torch.int64)
    order = torch.randperm(OP_E, generator=g)
    erow[order[:El]] = torch.randperm(El, generator=g)
    typed = order[El:]
    erow[typed] = El + torch.cat([torch.arange(T), torch.randint(0, T, (typed.numel() - T,), generator=g)])
    return ei, erow, El, T


OP_WIDTHS = [(1, 10), (1, 16), (3, 5), (4, 4), (4, 16), (8, 64), (1, 512), (2, 70)]


def _op_reference(heads, C, with_edge_rows):
    ei, erow, El, T = _op_graph(with_edge_rows)
    x, go = _inputs(OP_N, El, T, heads, C, seed=100 + heads * 1000 + C)
    o32 = _oracle(x, ei, erow, El, heads, go, torch.float32)
    o64 = _oracle(x, ei, erow, El, heads, go, torch.float64)
    x64 = {k: (None if v is None else v.double()) for k, v in x.items()}
    s = XO.logits(x64["q"], x64["k"], x64["e_edge"], x64["e_type"], ei, erow, El, heads)
    # the most-changing edge: of the twelve largest weights the one whose removal moves EVERY tensor most (an edge
    # that is its row's only in-edge moves out and dv alone: its ds is ~0)
    w = torch.exp(s.clamp(-5, 5)).max(1)[0]
    d64, best = None, -1.0
    for cand in torch.argsort(w, descending=True)[:12].tolist():
        c64 = _oracle(x, ei, erow, El, heads, go, torch.float64, skip=cand)
        score = min(_moved(c64, o64).values())
        if score > best:
            d64, best = c64, score
    expander_slot = int((erow == El + 1).nonzero()[0])
    w64 = _oracle(x, ei, erow, El, heads, go, torch.float64, swap=(expander_slot, El + 2))
    return x, go, ei, erow, El, T, o32, o64, s, d64, w64


def _moved(bad64, o64):
    """{tensor: max|bad - full| / max|full|} of a float64 run with one term changed."""
    return {k: float((bad64[k] - v).abs().max()) / float(v.abs().max()) for k, v in o64.items() if v is not None}


def _material(bad64, o64):
    """The tensors a changed term moves by more than 1e-3 of their scale -- a thousand times the referee's float32
    tolerance, so the referee must reject each of them -- as the dict ``teeth`` takes."""
    return {k: bad64[k] for k, m in _moved(bad64, o64).items() if m > 1e-3}


def _struct(ei, erow, rows, nv, El):
    # rows = num_nodes + num_graphs * nv; these hand-built unions are one "graph" whose last nv rows are virtual
    return ExphormerStructure.from_parts(ei.to(DEV), erow.to(DEV), rows - nv, 1, nv, El)


@pytest.mark.parametrize("with_edge_rows", [True, False], ids=["e_edge", "types-only"])
@pytest.mark.parametrize("heads,C", OP_WIDTHS)
def test_operator_on_a_multigraph_under_the_float64_referee(heads, C, with_edge_rows):
    what = f"exphormer attention H={heads} C={C} {'with' if with_edge_rows else 'without'} e_edge"
    x, go, ei, erow, El, T, o32, o64, s, d64, w64 = _op_reference(heads, C, with_edge_rows)
    assert float(s.abs().max()) < 4.0                        # far from the clamp
    assert bool((erow != torch.arange(OP_E)).any()) and set((erow[erow >= El] - El).tolist()) == set(range(T))
    struct = _struct(ei, erow, OP_N, OP_NV, El)
    got = _hip_run(x, struct, heads, go)
    referee_all(got, o32, o64, what)
    for k in ("out", "dq"):                                  # rows without in-edges
        assert not got[k][list(OP_ISOLATED)].any()
    for k in ("dk", "dv"):                                   # rows without out-edges
        assert not got[k][list(OP_ISOLATED)].any()
    for name, bad in (("most-changing edge removed", d64), ("an expander slot reads the node->virtual row", w64)):
        reached = _material(bad, o64)
        assert {"out", "dq", "dk", "dv", "de_type"} <= set(reached), (name, sorted(reached))
        teeth(got, o32, o64, reached, f"{what} [{name}]")


def test_operator_with_q_at_a_four_byte_offset():
    heads, C = 4, 16
    x, go, ei, erow, El, T, o32, o64, s, d64, w64 = _op_reference(heads, C, True)
    got = _hip_run(x, _struct(ei, erow, OP_N, OP_NV, El), heads, go, q_offset=True)
    referee_all(got, o32, o64, "exphormer attention, q misaligned")
    teeth(got, o32, o64, _material(d64, o64), "exphormer attention, q misaligned")


# --------------------------------------------------------------------------- #
# 3. long rows
# --------------------------------------------------------------------------- #
def _hub_graph(deg, seed, first=True, other=12):
    """A hub (row 0 of its graph of 41 rows) with ``deg`` in-edges and ``deg`` out-edges among 60 further edges, beside
    a second graph of ``other`` rows; ``first``: the hub's graph stands first.  The hub graph's edges keep their order."""
    g = torch.Generator().manual_seed(seed)
    n = 41
    peers = torch.randint(1, n, (deg,), generator=g)
    back = torch.randint(1, n, (deg,), generator=g)
    rest = torch.randint(1, n, (2, 60), generator=g)
    a = torch.cat([torch.stack([peers, torch.zeros(deg, dtype=torch.long)]),
                   torch.stack([torch.zeros(deg, dtype=torch.long), back]), rest], 1)
    a = a[:, torch.randperm(a.size(1), generator=g)]
    b = torch.randint(0, other, (2, 30), generator=g)
    T = 4
    erow_a = torch.randint(0, T, (a.size(1),), generator=g)
    erow_b = torch.randint(0, T, (30,), generator=g)
    if first:
        return torch.cat([a, b + n], 1).contiguous(), torch.cat([erow_a, erow_b]), n + other, 0
    return torch.cat([b, a + other], 1).contiguous(), torch.cat([erow_b, erow_a]), n + other, other


def _long_degrees():
    L = _hip.lib()
    long_row, chunk = L.hscn_exph_attn_long_row(), L.hscn_exph_attn_chunk()
    return long_row, chunk


@pytest.mark.parametrize("case", ["long", "long+1", "long+chunk+1", "rounds-wide", "rounds-narrow"])
def test_long_rows_in_both_walks_under_the_float64_referee(case):
    long_row, chunk = _long_degrees()
    # lane groups per workgroup = 256 / G: (1, 256) has G = 64 -> 4 groups, (2, 16) has G = 4 -> 64 groups
    heads, C, deg = {"long": (4, 4, long_row), "long+1": (4, 4, long_row + 1),
                     "long+chunk+1": (2, 16, long_row + chunk + 1),
                     "rounds-wide": (1, 256, long_row + chunk + 1),          # 6 chunks, 4 lane groups
                     "rounds-narrow": (2, 16, 64 * chunk + 1)}[case]         # 65 chunks, 64 lane groups
    assert case != "rounds-wide" or (deg + chunk - 1) // chunk > 256 // 64
    assert case != "rounds-narrow" or (deg + chunk - 1) // chunk > 256 // 4
    ei, erow, rows, hub = _hub_graph(deg, seed=deg)
    x, go = _inputs(rows, 0, 4, heads, C, seed=deg)
    assert int(torch.bincount(ei[1], minlength=rows)[hub]) == deg and int(torch.bincount(ei[0], minlength=rows)[hub]) == deg
    got = _hip_run(x, _struct(ei, erow, rows, 1, 0), heads, go)
    o32 = _oracle(x, ei, erow, 0, heads, go, torch.float32)
    o64 = _oracle(x, ei, erow, 0, heads, go, torch.float64)
    referee_all(got, o32, o64, f"hub of degree {deg}, H={heads} C={C}")
    hub_edge = int((ei[1] == hub).nonzero()[0])
    d64 = _oracle(x, ei, erow, 0, heads, go, torch.float64, skip=hub_edge)
    teeth(got, o32, o64, {k: d64[k] for k in ("out", "dq", "dk", "dv")}, f"hub of degree {deg}")


def test_a_hub_row_has_the_same_bits_wherever_its_graph_stands():
    long_row, chunk = _long_degrees()
    heads, C, deg = 2, 16, long_row + chunk + 1
    res = []
    for first in (True, False):
        ei, erow, rows, hub = _hub_graph(deg, seed=9, first=first)
        g = torch.Generator().manual_seed(1)
        xa = {k: torch.randn(41, heads * C, generator=g) for k in ("q", "k", "v")}
        xb = {k: torch.randn(12, heads * C, generator=g) for k in ("q", "k", "v")}
        x = {k: torch.cat([xa[k], xb[k]] if first else [xb[k], xa[k]]) for k in xa}
        x["e_edge"], x["e_type"] = None, torch.randn(4, heads * C, generator=g) * 0.5
        ga, gb = torch.randn(41, heads * C, generator=g), torch.randn(12, heads * C, generator=g)
        got = _hip_run(x, _struct(ei, erow, rows, 1, 0), heads, torch.cat([ga, gb] if first else [gb, ga]))
        res.append((got["out"][hub], got["dq"][hub], got["dk"][hub], got["dv"][hub]))
    for a, b in zip(*res):
        assert np.array_equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------- #
# 4. the table gradient
# --------------------------------------------------------------------------- #
def _type_counts():
    L = _hip.lib()
    long_row, chunk = L.hscn_exph_type_long_row(), L.hscn_exph_type_chunk()
    # nv = 4: ten types; type 0 has no slot
    return [0, 1, long_row, long_row + 1, 2 * chunk + 1, 3, 40, 2, 7, 5]


def _table_case(seed=21):
    counts = _type_counts()
    g = torch.Generator().manual_seed(seed)
    rows, El = 48, 30
    erow = torch.cat([torch.arange(El)] + [torch.full((c,), El + t) for t, c in enumerate(counts)])
    perm = torch.randperm(erow.numel(), generator=g)
    erow = erow[perm]
    ei = torch.randint(0, rows, (2, erow.numel()), generator=g)
    return ei, erow, rows, El, counts


def test_table_gradient_at_its_chunk_edges_under_the_float64_referee():
    heads, C = 4, 8
    ei, erow, rows, El, counts = _table_case()
    x, go = _inputs(rows, El, 10, heads, C, seed=4)
    struct = _struct(ei, erow, rows, 4, El)
    trowptr, titem = struct.type_slots
    assert (trowptr[1:] - trowptr[:-1]).tolist() == counts
    got = _hip_run(x, struct, heads, go)
    o32 = _oracle(x, ei, erow, El, heads, go, torch.float32)
    o64 = _oracle(x, ei, erow, El, heads, go, torch.float64)
    referee_all(got, o32, o64, "table gradient")
    assert not got["de_type"][0].any() and not o64["de_type"][0].any()          # a type without slots: exact zeros
    for t in (1, 2, 3, 4):                                                        # each type by itself
        referee_all({"row": got["de_type"][t]}, {"row": o32["de_type"][t]}, {"row": o64["de_type"][t]}, f"type {t}")
        slot = int((erow == El + t).nonzero()[0])
        d64 = _oracle(x, ei, erow, El, heads, go, torch.float64, skip=slot)
        teeth({"row": got["de_type"][t]}, {"row": o32["de_type"][t]}, {"row": o64["de_type"][t]},
              {"row": d64["de_type"][t]}, f"type {t}")
    again = _hip_run(x, _struct(ei, erow, rows, 4, El), heads, go)
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k


def test_only_what_needs_a_gradient_is_computed():
    heads, C = 4, 8
    ei, erow, rows, El, _ = _table_case()
    x, go = _inputs(rows, El, 10, heads, C, seed=4)
    struct = _struct(ei, erow, rows, 4, El)
    full = _hip_run(x, struct, heads, go)
    for only in ("q", "k", "v", "e_edge", "e_type"):
        t = {k: v.to(DEV).requires_grad_(k == only) for k, v in x.items()}
        out = Fh.ExphormerAttentionFn.apply(t["q"], t["k"], t["v"], t["e_edge"], t["e_type"], struct, heads)
        out.backward(go.to(DEV))
        key = {"e_edge": "de_edge", "e_type": "de_type"}.get(only, "d" + only)
        assert np.array_equal(_bits(t[only].grad), _bits(full[key])), only
        assert all(t[k].grad is None for k in t if k != only)


# --------------------------------------------------------------------------- #
# 5. the clamp
# --------------------------------------------------------------------------- #
CLAMP_HEADS, CLAMP_C, CLAMP_SEED = 4, 4, 0


def _clamp_reference(seed):
    """The multigraph of section 2 with every input x 3: float64 logits saturate on both sides.  Returns the inputs and
    the float64 logits' margins (the seed search reads them alone)."""
    ei, erow, El, T = _op_graph(True)
    x, go = _inputs(OP_N, El, T, CLAMP_HEADS, CLAMP_C, seed=seed, scale=3.0)
    x64 = {k: (None if v is None else v.double()) for k, v in x.items()}
    s = XO.logits(x64["q"], x64["k"], x64["e_edge"], x64["e_type"], ei, erow, El, CLAMP_HEADS)
    E = OP_E
    ee = XO.edge_rows(x64["e_edge"], x64["e_type"], erow, El).view(E, CLAMP_HEADS, CLAMP_C)
    mag = (x64["q"][ei[1]].view(E, CLAMP_HEADS, CLAMP_C) * x64["k"][ei[0]].view(E, CLAMP_HEADS, CLAMP_C) * ee).abs().sum(-1)
    bound = (CLAMP_C + 2) * 2.0 ** -24 / math.sqrt(CLAMP_C) * mag
    return x, go, ei, erow, El, s, bound


def test_clamp_gates_the_gradients_on_both_sides():
    x, go, ei, erow, El, s, bound = _clamp_reference(CLAMP_SEED)
    n = s.numel()
    assert int((s > 5).sum()) >= 0.05 * n and int((s < -5).sum()) >= 0.05 * n
    assert int((s.abs() < 5).sum()) >= 0.20 * n
    assert float((s.abs() - 5).abs().min()) > 1e-3          # no logit near a bound ...
    assert float(bound.max()) < 1e-4                        # ... and float32 is this close: both take the same side
    struct = _struct(ei, erow, OP_N, OP_NV, El)
    got = _hip_run(x, struct, CLAMP_HEADS, go)
    o32 = _oracle(x, ei, erow, El, CLAMP_HEADS, go, torch.float32)
    o64 = _oracle(x, ei, erow, El, CLAMP_HEADS, go, torch.float64)
    referee_all(got, o32, o64, "clamped attention")
    own = (erow < El).nonzero().flatten()
    saturated = s[own].abs() > 5                            # [own edges, heads]
    de = got["de_edge"][erow[own]].view(own.numel(), CLAMP_HEADS, CLAMP_C).cpu()
    assert bool(saturated.any()) and not de[saturated].any()
    assert bool(de[~saturated].any())
    assert not o64["de_edge"][erow[own]].view(own.numel(), CLAMP_HEADS, CLAMP_C)[saturated].any()


# --------------------------------------------------------------------------- #
# 6. the model
# --------------------------------------------------------------------------- #
M_F, M_D, M_C, M_L, M_HEADS, M_DE, M_DEGREE = 6, 16, 8, 2, 4, 3, 2      # (the pair decoder takes widths 4 k)
M_SIZES = (5, 9, 7)
M_CASES = [(lvl, conv, nv) for lvl in ("graph", "node", "link") for conv in (None, "gine") for nv in (0, 1)]
# (task level, local_conv, nv) -> seed: the first of the seeds 0, 1, ... whose float64 run meets the gate condition of
# tests/test_gpu_attention.py with half as much again to spare (``_gate_margin`` > 1.5: every ReLU input farther from
# zero than 6 x the referee's limit for its tensor).  A CPU-only choice: ``_model_reference`` runs no product code.
M_SEEDS = {case: 0 for case in M_CASES}            # (seed 0 has 15 x .. 178 x to spare in every case)


def _model_batch(seed, conv, level):
    g = torch.Generator().manual_seed(500 + seed)
    graphs = []
    for n in M_SIZES:
        half = torch.randint(0, n, (2, n + 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        d = Data(x=torch.randn(n, M_F, generator=g), edge_index=ei, y=torch.zeros(1, M_C))
        if conv == "gine":
            d.edge_attr = torch.randn(ei.size(1), M_DE, generator=g)
        if level == "link":
            pairs = torch.randperm(n * n, generator=g)[:6]
            d.edge_label_index = torch.stack([pairs // n, pairs % n])
            d.edge_label = torch.randint(0, 2, (6,), generator=g).float()
        graphs.append(d)
    return Batch.from_data_list(graphs)


def _model_run(ref, b, union, gy, dtype, skip=None):
    m = copy.deepcopy(ref).to(dtype)
    seen = {}
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    ea = getattr(b, "edge_attr", None)
    pairs = b.edge_label_index if m.task_level == "link" else None
    out = m(b.x.to(dtype), b.edge_index, None if ea is None else ea.to(dtype), b.batch, int(b.num_graphs), union, pairs,
            skip)
    out.backward(gy.to(dtype))
    grads = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()
             if p.numel()}
    return grads, out.detach(), seen


def _model_reference(level, conv, nv, seed):
    b = _model_batch(seed, conv, level)
    torch.manual_seed(seed)
    ref = XO.ExphormerGPSRef(M_F, M_D, M_C, M_L, M_HEADS, conv, nv, level, M_DE if conv == "gine" else None)
    ex = XO.expander_edges(list(M_SIZES), M_DEGREE, 0, list(range(len(M_SIZES))))
    union = XO.union_graph(b.edge_index, b.batch, int(b.num_graphs), ex, nv, True, conv == "gine")
    rows = {"graph": (len(M_SIZES), M_C), "node": (sum(M_SIZES), M_C)}.get(level) or (int(b.edge_label_index.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))
    r32 = _model_run(ref, b, union, gy, torch.float32)
    r64 = _model_run(ref, b, union, gy, torch.float64)
    d64 = _model_run(ref, b, union, gy, torch.float64, skip=int(union[0].size(1)) - 1)     # the last union edge
    return ref, b, union, gy, r32, r64, d64


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


@pytest.mark.parametrize("level,conv,nv", M_CASES)
def test_gps_with_exphormer_under_the_float64_referee(level, conv, nv):
    from graph_hscn.train import batching
    what = f"GPS exphormer {level} level, local_conv={conv}, nv={nv}"
    seed = M_SEEDS[(level, conv, nv)]
    ref, b, union, gy, (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = _model_reference(level, conv, nv, seed)
    assert len(g64) == M_L * (3 if conv == "gine" else 1) + 1
    _check_gates(g32, g64, what)
    pm = GPS(M_F, M_D, M_C, M_L, M_HEADS, conv, ACT_DICT["relu"], 0.0, "layer", level, global_model="exphormer",
             expander_degree=M_DEGREE, num_virtual_nodes=nv, add_local_edges=True, expander_seed=0).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    if conv == "gine":
        for layer in pm.layers:
            layer.conv.lin.materialize(M_DE, bd.x)
        pm.exph_edge_encoder.materialize(M_DE, bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    back = copy.deepcopy(ref)                               # and the other way round
    back.load_state_dict({k: v.detach().cpu().clone() for k, v in pm.state_dict().items()}, strict=True)
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in ref.state_dict().items())
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    pm.check_flags()
    # the structure the model built is the restatement's union graph, and it is kept on the batch
    struct = ExphormerStructure.of(bd, M_DEGREE, nv, True, 0, edge_features=conv == "gine")
    assert torch.equal(struct.edge_index.cpu(), union[0]) and struct.erow.cpu().tolist() == union[1].tolist()
    assert struct is ExphormerStructure.of(bd, M_DEGREE, nv, True, 0, edge_features=conv == "gine")
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dy64}, what)
    got = {k: v for k, v in grads_of(pm).items() if k in o64}
    assert set(got) == set(o64)
    referee_all(got, o32, o64, what)
    reached = _material(d64, o64)
    assert {"p.node_encoder.weight", "p.layers.0.attn.Q.weight", "p.layers.0.attn.E.weight",
            "p.edge_type_emb.weight"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what)
