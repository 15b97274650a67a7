"""GCNII on the device: the one-launch GCN2Conv operator and its backward against tests/gcn2_oracle.py under the float64
referee (``referee_all`` / ``teeth`` of tests/helpers.py: the float32 and float64 restatements are the two oracles, no
constant of this file's own) on a built graph at the tile, panel and structure edges; the exact facts; the launch
counts; ``GCN2Conv`` against ``GCNConv``; the ``GCNII`` model at the three task levels; one ``train.train`` epoch.

Everything a case computes on the CPU sits in a function of its own (``_op_reference``, ``_model_reference``): the
conditions on the data are asserted there, on the float64 run, and the seeds below were chosen by running those alone."""
import copy
import functools
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, RWSEConfig
from graph_hscn.data import Batch, Data, DataLoader
from graph_hscn.encoder.categorical import ATOM_FEATURE_DIMS
from graph_hscn.model.gcnii import GCNII
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GCN2Conv, GCNConv
from graph_hscn.structure import self_loop_relation_of
from tests import gcn2_oracle as GO
from tests.helpers import DEV, KinkGuard, grads_of, referee, referee_all, teeth

pytestmark = pytest.mark.gpu

KEYS = ("out", "g_x", "g_x0", "g_W1", "g_W2")
BETA_DEEP = math.log(0.5 / 64 + 1.0)          # layer 64 under theta = 0.5
ACT = _hip.ACT


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------- #
# the built graph
# --------------------------------------------------------------------------- #
HUB_ROW = 300                                  # the gather has no long-row constant: one hub whose row holds 300 slots
BUILT_N = 301                                  # 9 tiles of 32 + 13 rows, 18 tiles of 16 + 13 rows
LONER, ONE_IN, TWICE, OWN_LOOP, HUB, SENDER = 0, 1, 2, 3, 4, 5
EDGE_INTO_ONE_IN = "the edge into the node with one in-edge"


@functools.lru_cache(maxsize=None)
def _built_graph():
    """(edge_index [2, E] shuffled, the listed id of the edge 7 -> ONE_IN)."""
    g = torch.Generator().manual_seed(5)
    rest = list(range(6, BUILT_N))
    edges = [(7, ONE_IN), (8, TWICE), (8, TWICE), (OWN_LOOP, OWN_LOOP), (9, OWN_LOOP), (10, OWN_LOOP)]
    edges += [(j, HUB) for j in [ONE_IN, TWICE, OWN_LOOP, SENDER] + rest]                  # 299 in-edges + its loop
    edges += [(SENDER, t) for t in rest] + [(SENDER, t) for t in (6, 7, 8)]                # 298 + the hub's + its loop
    a = torch.randint(6, BUILT_N, (2, 600), generator=g)
    edges += list(zip(a[0].tolist(), a[1].tolist()))                                       # (loops and repeats as they fall)
    ei = torch.tensor(edges, dtype=torch.long).t().contiguous()
    perm = torch.randperm(ei.size(1), generator=g)
    where = torch.empty_like(perm)
    where[perm] = torch.arange(perm.numel())
    return ei[:, perm].contiguous(), int(where[0])


def test_the_built_graph_holds_what_it_says():
    ei, e_one = _built_graph()
    full, _ = GO.with_loops(ei, BUILT_N)
    row = torch.bincount(full[1], minlength=BUILT_N)
    sent = torch.bincount(full[0], minlength=BUILT_N)
    assert int(row[LONER]) == 1 and int(sent[LONER]) == 1                  # its loop is its only slot
    assert int(row[ONE_IN]) == 2 and tuple(ei[:, e_one].tolist()) == (7, ONE_IN)
    assert int(((ei[0] == 8) & (ei[1] == TWICE)).sum()) == 2 and int(row[TWICE]) == 3
    assert int(((ei[0] == OWN_LOOP) & (ei[1] == OWN_LOOP)).sum()) == 1 and int(row[OWN_LOOP]) == 3
    assert int(row[HUB]) == HUB_ROW and int(sent[SENDER]) == HUB_ROW
    assert BUILT_N % Fh.GCN2_ROW_TILE and BUILT_N % Fh.GCN2_ROW_TILE_TWO and BUILT_N > 2 * Fh.GCN2_ROW_TILE
    assert not torch.equal(ei[1], ei[1].sort()[0])                          # shuffled: a row's slots are not its edge ids


# --------------------------------------------------------------------------- #
# one oracle evaluation, one HIP evaluation
# --------------------------------------------------------------------------- #
def _inputs(N, H, shared, seed):
    g = torch.Generator().manual_seed(seed)
    t = {"x": torch.randn(N, H, generator=g), "x0": torch.randn(N, H, generator=g),
         "W1": torch.randn(H, H, generator=g) / math.sqrt(H),
         "W2": None if shared else torch.randn(H, H, generator=g) / math.sqrt(H)}
    return t, torch.randn(N, H, generator=g)


def _oracle(t, ei, alpha, beta, act, go, dtype, skip=None):
    v = {k: (None if a is None else a.detach().clone().to(dtype).requires_grad_(True)) for k, a in t.items()}
    out = GO.gcn2(v["x"], v["x0"], ei, v["W1"], v["W2"], alpha, beta, act, skip)
    out.backward(go.to(dtype))
    return {"out": out.detach(), "g_x": v["x"].grad, "g_x0": v["x0"].grad, "g_W1": v["W1"].grad,
            "g_W2": None if v["W2"] is None else v["W2"].grad}


def _hip_run(t, ei, alpha, beta, act, go, need=("x", "x0", "W1", "W2")):
    N = t["x"].size(0)
    v = {k: (None if a is None else a.detach().clone().to(DEV).requires_grad_(k in need)) for k, a in t.items()}
    rel = self_loop_relation_of(ei.to(DEV), N, both=True)
    out = Fh.GCN2ConvFn.apply(v["x"], v["x0"], v["W1"], v["W2"], rel, alpha, beta, ACT[act])
    if out.requires_grad:
        out.backward(go.to(DEV))
    rel.check()
    return {"out": out.detach(), "g_x": v["x"].grad, "g_x0": v["x0"].grad, "g_W1": v["W1"].grad,
            "g_W2": None if v["W2"] is None else v["W2"].grad}


def _bar(v32, v64):
    """The referee's limit for a tensor with these two oracle evaluations."""
    return 2.0 * float((v32.double() - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())


def _reference(t, go, ei, alpha, beta, act, skip):
    """The float32 and float64 runs, the float64 run with one edge skipped, and the cotangent that was used: with a ReLU
    the cotangent is zeroed wherever the float64 pre-activation comes within 8 x the forward bar of zero, so that no
    gate that carries a gradient can differ between HIP, float32 and float64 (asserted KinkGuard's way, on float64)."""
    if act == "relu":
        y32 = GO.gcn2(t["x"], t["x0"], ei, t["W1"], t["W2"], alpha, beta)
        y64 = GO.gcn2(*(None if a is None else a.double() for a in (t["x"], t["x0"])), ei, t["W1"].double(),
                      None if t["W2"] is None else t["W2"].double(), alpha, beta)
        bar = _bar(y32, y64)
        go = go * (y64.abs() > 8.0 * bar).to(go.dtype)
        live = y64[go != 0]
        assert live.numel() > 0.9 * y64.numel() and int((live < 0).sum()) > 0.2 * live.numel()
        kg = KinkGuard()
        kg.watch("GCN2Conv pre-activation with a cotangent", live)
        kg.check(bar, what="GCN2Conv")
    o32 = _oracle(t, ei, alpha, beta, act, go, torch.float32)
    o64 = _oracle(t, ei, alpha, beta, act, go, torch.float64)
    for k, v in o64.items():                       # no tensor that cancels to nothing (exact zeros are said so below)
        zero = (k == "g_x" and alpha == 1.0) or (k in ("g_x0", "g_W2") and alpha == 0.0)
        if v is not None:
            assert (not v.any()) if zero else float(v.abs().max()) > 1e-3, k
    d64 = None if skip is None else _oracle(t, ei, alpha, beta, act, go, torch.float64, skip=skip)
    return go, o32, o64, d64


def _edge_width(which, shared):
    edge = Fh.gcn2_resident_max_width(shared)
    return {"edge": edge, "edge+4": edge + 4}.get(which, which)


# every value of alpha, beta, shared_weights and act with every width
OP_WIDTHS = (4, 20, "edge", "edge+4", 300, 512)
OP_SETTINGS = ((0.0, 1.0, True, "identity"), (0.1, BETA_DEEP, False, "relu"), (1.0, BETA_DEEP, True, "relu"),
               (0.1, 1.0, False, "identity"))


@functools.lru_cache(maxsize=None)
def _op_reference(width, alpha, beta, shared, act):
    H = _edge_width(width, shared)
    ei, e_one = _built_graph()
    t, go = _inputs(BUILT_N, H, shared, seed=1000 + H + (0 if shared else 7))
    go, o32, o64, d64 = _reference(t, go, ei, alpha, beta, act, e_one)
    return H, t, go, ei, o32, o64, d64


@pytest.mark.parametrize("alpha,beta,shared,act", OP_SETTINGS)
@pytest.mark.parametrize("width", OP_WIDTHS)
def test_operator_on_the_built_graph_under_the_float64_referee(width, alpha, beta, shared, act):
    H, t, go, ei, o32, o64, d64 = _op_reference(width, alpha, beta, shared, act)
    plan = Fh.gcn2_plan(H, shared)
    if width == "edge":
        assert plan["resident"] and not Fh.gcn2_plan(H + 4, shared)["resident"]
    what = f"GCN2Conv H={H} alpha={alpha} beta={beta:.4f} shared={shared} {act} (panel {plan['panel']})"
    got = _hip_run(t, ei, alpha, beta, act, go)
    referee_all(got, o32, o64, what)
    for rows, name in (([LONER], "its loop only"), ([ONE_IN], "one in-edge"), ([TWICE], "an edge twice"),
                       ([OWN_LOOP], "a listed self loop"), ([HUB], "the hub"), ([SENDER], "the sender")):
        sub = lambda d: {k: d[k][rows] for k in ("out", "g_x", "g_x0")}
        referee_all(sub(got), sub(o32), sub(o64), f"{what}, {name}")
    if alpha == 1.0:                               # the propagated term does not enter: nothing for the teeth to drop
        assert all(torch.equal(d64[k], o64[k]) for k in ("out", "g_x", "g_W1"))
        assert not got["g_x"].any()
        return
    moved = {k: float((d64[k] - o64[k]).abs().max()) / float(o64[k].abs().max()) for k in ("out", "g_x", "g_W1")}
    assert all(m > 1e-4 for m in moved.values()), moved       # a hundred times the referee's float32 tolerance
    teeth(got, o32, o64, {k: d64[k] for k in ("out", "g_x", "g_W1")}, f"{what} [{EDGE_INTO_ONE_IN} dropped]")


def _small_graph(N, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, 3 * N), generator=g)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


@functools.lru_cache(maxsize=None)
def _tile_reference(N, shared):
    ei = _small_graph(N, seed=40 + N)
    skip = int((ei[0] != ei[1]).nonzero()[0])
    t, go = _inputs(N, 20, shared, seed=50 + N)
    return (t, ei) + _reference(t, go, ei, 0.1, BETA_DEEP, "relu", skip)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("shared", [True, False])
def test_one_row_tile_and_one_row_more(shared, extra):
    N = (Fh.GCN2_ROW_TILE if shared else Fh.GCN2_ROW_TILE_TWO) + extra
    assert N == Fh.gcn2_plan(20, shared)["row_tile"] + extra
    t, ei, go, o32, o64, d64 = _tile_reference(N, shared)
    got = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go)
    what = f"GCN2Conv N={N} shared={shared}"
    referee_all(got, o32, o64, what)
    teeth(got, o32, o64, {k: d64[k] for k in ("out", "g_x")}, what)


# --------------------------------------------------------------------------- #
# exact facts
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("shared", [True, False])
def test_alpha_one_does_not_read_x_and_gives_exact_zeros_for_its_gradient(shared):
    ei, _ = _built_graph()
    t, go = _inputs(BUILT_N, 20, shared, seed=61)
    a = _hip_run(t, ei, 1.0, BETA_DEEP, "relu", go)
    b = _hip_run(dict(t, x=t["x"] * 3.0 + 1.0), ei, 1.0, BETA_DEEP, "relu", go)
    assert np.array_equal(_bits(a["out"]), _bits(b["out"]))
    assert a["g_x"].shape == t["x"].shape and not _bits(a["g_x"]).any()        # +0.0 everywhere
    assert bool(a["g_x0"].any())
    if shared:
        assert bool(a["g_W1"].any())
    else:                                          # weight1 multiplies (1 - alpha) p = 0: x0 reaches out through weight2
        assert not a["g_W1"].any() and bool(a["g_W2"].any())


def test_only_what_needs_a_gradient_gets_one():
    ei, _ = _built_graph()
    t, go = _inputs(BUILT_N, 20, False, seed=62)
    full = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go)
    key = {"x": "g_x", "x0": "g_x0", "W1": "g_W1", "W2": "g_W2"}
    for only in key:
        got = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go, need=(only,))
        assert np.array_equal(_bits(got[key[only]]), _bits(full[key[only]])), only
        assert all(got[key[n]] is None for n in key if n != only), only
    none = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go, need=())
    assert np.array_equal(_bits(none["out"]), _bits(full["out"])) and all(none[k] is None for k in key.values())


@pytest.mark.parametrize("H,shared", [(20, True), (132, True), (100, False)])
def test_two_runs_give_the_same_bits(H, shared):
    ei, _ = _built_graph()
    t, go = _inputs(BUILT_N, H, shared, seed=63)
    first = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go)
    again = _hip_run(t, ei, 0.1, BETA_DEEP, "relu", go)
    for k in KEYS:
        if first[k] is None:
            assert again[k] is None and shared and k == "g_W2"
        else:
            assert np.array_equal(_bits(first[k]), _bits(again[k])), k


# --------------------------------------------------------------------------- #
# against GCNConv; launch counts; empty cases
# --------------------------------------------------------------------------- #
def test_alpha_zero_beta_one_is_gcnconv_without_bias():
    H = 20
    ei, _ = _built_graph()
    t, go = _inputs(BUILT_N, H, True, seed=71)
    go, o32, o64, _ = _reference(t, go, ei, 0.0, 1.0, "identity", None)
    got = _hip_run(t, ei, 0.0, 1.0, "identity", go)
    conv = GCNConv(H, H, bias=False).to(DEV)
    with torch.no_grad():
        conv.lin.weight.copy_(t["W1"].t())
    x = t["x"].clone().to(DEV).requires_grad_(True)
    out = conv(x, ei.to(DEV))
    out.backward(go.to(DEV))
    for k, other in (("out", out), ("g_x", x.grad)):         # two float32 evaluations of A_hat x W1 in different orders
        assert referee(got[k], o32[k], o64[k], f"GCN2Conv {k}") <= 1.0
        assert referee(other, o32[k], o64[k], f"GCNConv {k}") <= 1.0


class _CallSpy:
    """Names issued through ``_hip.call`` (under either of the names the operators call it by) while active."""

    def __init__(self, monkeypatch):
        self.names = []
        real = _hip.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(_hip, "call", call)
        monkeypatch.setattr(Fh, "call", call)


@pytest.mark.parametrize("H,shared", [(20, True), (300, True), (20, False), (300, False)])
def test_a_layer_is_one_launch_forward_and_at_most_three_calls_backward(H, shared, monkeypatch):
    ei, _ = _built_graph()
    t, go = _inputs(BUILT_N, H, shared, seed=72)
    conv = GCN2Conv(H, 0.1, 0.5, 3, shared_weights=shared).to(DEV)
    rel = self_loop_relation_of(ei.to(DEV), BUILT_N, both=True)
    rel.dinv                                                  # the structure is the model's to build, once per forward
    x, x0 = t["x"].to(DEV).requires_grad_(True), t["x0"].to(DEV).requires_grad_(True)
    spy = _CallSpy(monkeypatch)
    out = conv(x, x0, rel, act="relu")
    assert spy.names == ["hscn_gcn2_fwd"]
    del spy.names[:]
    out.backward(go.to(DEV))
    assert len(spy.names) <= 3 and spy.names == ["hscn_gcn2_bwd", "hscn_gcn2_bwd_w", "hscn_spmm_csr_gcn"], spy.names
    assert not any(n.startswith("hscn_linear") or n.startswith("hscn_act") for n in spy.names)
    del spy.names[:]
    with torch.no_grad():
        conv(x, x0, ei.to(DEV))                               # an edge list: the relation is cached from above
    assert [n for n in spy.names if n.startswith("hscn_gcn2_")] == ["hscn_gcn2_fwd"]


def test_no_nodes_is_no_call(monkeypatch):
    conv = GCN2Conv(20, 0.1, shared_weights=False).to(DEV)
    x = torch.zeros(0, 20, device=DEV, requires_grad=True)
    spy = _CallSpy(monkeypatch)
    out = conv(x, torch.zeros(5, 20, device=DEV), torch.zeros(2, 0, dtype=torch.long, device=DEV), act="relu")
    assert tuple(out.shape) == (0, 20) and spy.names == []
    out.sum().backward()
    assert spy.names == [] and tuple(x.grad.shape) == (0, 20)
    assert not conv.weight1.grad.any() and not conv.weight2.grad.any()


@pytest.mark.parametrize("shared", [True, False])
def test_loops_only_propagates_x_itself(shared):
    N, H = 37, 20
    ei = torch.zeros(2, 0, dtype=torch.long)
    t, go = _inputs(N, H, shared, seed=73)
    go, o32, o64, _ = _reference(t, go, ei, 0.25, BETA_DEEP, "identity", None)
    assert torch.equal(GO.propagate(t["x"].double(), ei), t["x"].double())           # p = x: every degree is 1
    got = _hip_run(t, ei, 0.25, BETA_DEEP, "identity", go)
    referee_all(got, o32, o64, f"GCN2Conv without edges, shared={shared}")


# --------------------------------------------------------------------------- #
# the model
# --------------------------------------------------------------------------- #
M_F, M_H, M_C, M_L, M_K, M_PE = 6, 20, 8, 4, 6, 4               # (the pair decoder takes widths 4 k)
M_SIZES = (5, 9, 1, 7, 33, 6)
M_CASES = [("graph", False, "rwse"), ("node", True, "atom"), ("link", False, "linear"), ("graph", True, "linear")]
# case -> seed: the first of the seeds 0, 1, ... whose float64 run meets the gate condition (``_gate_margin`` > 1.5:
# every ReLU input farther from zero than 6 x the referee's limit for its tensor).  A CPU-only choice:
# ``_model_reference`` runs no product code.
M_SEEDS = {case: 0 for case in M_CASES}
DROPOUT_P, DROPOUT_SEED, DROPOUT_CASE_SEED = 0.2, 11, 0


def _model_batch(seed, enc, level):
    g = torch.Generator().manual_seed(800 + seed)
    graphs = []
    for n in M_SIZES:
        half = torch.randint(0, n, (2, n + 2), generator=g)
        ei = torch.cat([half, half.flip(0)], 1)
        if enc == "atom":
            d = Data(x=torch.stack([torch.randint(0, c, (n,), generator=g) for c in ATOM_FEATURE_DIMS], 1), edge_index=ei,
                     y=torch.zeros(1, M_C))
        else:
            d = Data(x=torch.randn(n, M_F, generator=g), edge_index=ei, y=torch.zeros(1, M_C))
        d.edge_attr = torch.randn(ei.size(1), 3, generator=g)                  # carried and not read
        if enc == "rwse":
            d.rwse = torch.rand(n, M_K, generator=g)
        if level == "link":
            pairs = torch.randperm(n * n, generator=g)[:min(6, n * n)]
            d.edge_label_index = torch.stack([pairs // n, pairs % n])
            d.edge_label = torch.randint(0, 2, (pairs.numel(),), generator=g).float()
        graphs.append(d)
    return Batch.from_data_list(graphs)


def _ref_model(level, residual, enc):
    return GO.GCNIIRef(M_F, M_H, M_C, M_L, 0.1, 0.5, True, residual, level,
                       node_encoder=ATOM_FEATURE_DIMS if enc == "atom" else None,
                       rwse=(M_K, M_PE) if enc == "rwse" else None)


def _model_run(ref, b, gy, dtype, skip=None, masks=None, scale=1.0):
    m = copy.deepcopy(ref).to(dtype)
    seen = {}
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    x = b.x.to(dtype) if b.x.is_floating_point() else b.x
    stats = b.rwse.to(dtype) if hasattr(m, "pe_encoder") else None
    out = m(x, b.edge_index, b.batch, len(M_SIZES), b.edge_label_index if m.task_level == "link" else None, stats, skip,
            masks, scale)
    out.backward(gy.to(dtype))
    grads = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    return grads, out.detach(), seen


def _rows(level, b):
    return {"graph": (len(M_SIZES), M_C), "node": (sum(M_SIZES), M_C)}.get(level) or (int(b.edge_label_index.size(1)),)


@functools.lru_cache(maxsize=None)
def _model_reference(level, residual, enc, seed):
    b = _model_batch(seed, enc, level)
    torch.manual_seed(seed)
    ref = _ref_model(level, residual, enc)
    gy = torch.randn(*_rows(level, b), generator=torch.Generator().manual_seed(1))
    skip = int(((b.edge_index[0] != b.edge_index[1]) & (b.edge_index[1] >= int(b.ptr[1]))).nonzero()[0])
    r32, r64 = _model_run(ref, b, gy, torch.float32), _model_run(ref, b, gy, torch.float64)
    assert _gate_margin(r32[2], r64[2]) > 1.5, (level, residual, enc, seed)       # the rule the seed was chosen by
    return ref, b, gy, r32, r64, _model_run(ref, b, gy, torch.float64, skip=skip)


def _gate_margin(g32, g64):
    """min over the ReLU inputs of |value| / (4 x the referee's limit of its tensor): > 1 meets the gate condition."""
    return min(float(v64.abs().min()) / (4.0 * _bar(g32[tag], v64)) for tag, v64 in g64.items())


def _check_gates(g32, g64, what):
    assert set(g32) == set(g64) and len(g64) == M_L + 1
    for tag, v64 in g64.items():
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(_bar(g32[tag], v64), what=f"{what} {tag}")


def _product_model(level, residual, enc, dropout=0.0):
    pe = RWSEConfig(dim_in=M_F, dim_emb=M_H, dim_pe=M_PE, ksteps=M_K) if enc == "rwse" else None
    return GCNII(9 if enc == "atom" else M_F, M_H, M_C, M_L, ACT_DICT["relu"], dropout, 0.1, 0.5, True, residual, level,
                 "atom" if enc == "atom" else None, pe).to(DEV)


def _load(pm, ref):
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    back = copy.deepcopy(ref)                               # and the other way round
    back.load_state_dict({k: v.detach().cpu().clone() for k, v in pm.state_dict().items()}, strict=True)
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in ref.state_dict().items())


def _material(bad64, o64):
    """The tensors a removed edge moves by more than 1e-3 of their scale, as the dict ``teeth`` takes."""
    return {k: bad64[k] for k, v in o64.items() if v is not None and v.numel() and
            float((bad64[k] - v).abs().max()) > 1e-3 * float(v.abs().max())}


@pytest.mark.parametrize("level,residual,enc", M_CASES)
def test_gcnii_model_under_the_float64_referee(level, residual, enc):
    from graph_hscn.train import batching
    what = f"GCNII {level} level, residual={residual}, {enc}"
    ref, b, gy, (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = \
        _model_reference(level, residual, enc, M_SEEDS[(level, residual, enc)])
    _check_gates(g32, g64, what)
    pm = _product_model(level, residual, enc)
    _load(pm, ref)
    bd = batching.to_device(pm, b, DEV)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    pm.check_flags()
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dy64}, what + " [an edge dropped]")
    got = grads_of(pm)
    assert set(got) == set(o64) and all(v is not None for v in o64.values())
    referee_all(got, o32, o64, what)
    reached = _material(d64, o64)
    assert {"p.node_encoder.weight", "p.layers.0.weight1", f"p.layers.{M_L - 1}.weight1"} <= set(reached), sorted(reached)
    teeth(got, o32, o64, reached, what + " [an edge dropped]")


@functools.lru_cache(maxsize=None)
def _dropout_reference(seed):
    from tests.test_gpu_exact_edges import keep_mask
    level, residual, enc = "node", True, "linear"
    b = _model_batch(seed, enc, level)
    torch.manual_seed(seed)
    ref = _ref_model(level, residual, enc)
    gy = torch.randn(*_rows(level, b), generator=torch.Generator().manual_seed(1))
    N = sum(M_SIZES)
    masks = [torch.from_numpy(keep_mask(N * M_H, DROPOUT_P, DROPOUT_SEED + l).reshape(N, M_H)) for l in range(1, M_L + 1)]
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(DROPOUT_P)))
    return ref, b, gy, masks, _model_run(ref, b, gy, torch.float32, masks=masks, scale=scale), \
        _model_run(ref, b, gy, torch.float64, masks=masks, scale=scale)


def test_gcnii_with_pinned_dropout_masks_equals_the_philox_restatement():
    from graph_hscn.train import batching
    what = f"GCNII with dropout {DROPOUT_P} under seed {DROPOUT_SEED}"
    ref, b, gy, masks, (o32, y32, g32), (o64, y64, g64) = _dropout_reference(DROPOUT_CASE_SEED)
    kept = float(torch.stack(masks).float().mean())
    assert 0.7 < kept < 0.9 and not torch.equal(masks[0], masks[1])
    _check_gates(g32, g64, what)
    pm = _product_model("node", True, "linear", dropout=DROPOUT_P)
    _load(pm, ref)
    pm.train()
    pm.dropout_seed = DROPOUT_SEED
    pred = pm(batching.to_device(pm, b, DEV))
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    referee_all(grads_of(pm), o32, o64, what)
    pm.eval()
    with torch.no_grad():                                       # not training: no mask
        plain = pm(batching.to_device(pm, b, DEV))
    assert not torch.equal(plain, pred.detach())


@functools.lru_cache(maxsize=None)
def _pool_reference(H):
    b = _model_batch(0, "linear", "graph")
    g = torch.Generator().manual_seed(90 + H)
    x, gy = torch.randn(sum(M_SIZES), H, generator=g), torch.randn(len(M_SIZES), H, generator=g)

    def run(dtype):
        t = x.clone().to(dtype).requires_grad_(True)
        sums = torch.zeros(len(M_SIZES), H, dtype=dtype).index_add_(0, b.batch, t)
        out = sums / torch.bincount(b.batch, minlength=len(M_SIZES)).to(dtype).unsqueeze(1)
        out.backward(gy.to(dtype))
        return {"pooled": out.detach(), "g_x": t.grad}
    return b, x, gy, run(torch.float32), run(torch.float64)


@pytest.mark.parametrize("H", [256, 260, 300, 512])
def test_the_graph_level_pools_the_whole_envelope_in_column_slices(H):
    from graph_hscn.model.gcnii import POOL_MAX_WIDTH
    from graph_hscn.train import batching
    assert H in (POOL_MAX_WIDTH, POOL_MAX_WIDTH + 4) or H > POOL_MAX_WIDTH
    b, x, gy, o32, o64 = _pool_reference(H)
    pm = GCNII(M_F, H, M_C, 1).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    t = x.clone().to(DEV).requires_grad_(True)
    out = pm._pool(t, bd)
    out.backward(gy.to(DEV))
    referee_all({"pooled": out, "g_x": t.grad}, o32, o64, f"GCNII's mean pool at H={H}")
    o64_cut = {"pooled": o64["pooled"].clone()}
    o64_cut["pooled"][4, H - 1] -= x[int(b.ptr[4]), H - 1].double() / M_SIZES[4]     # one node of the last column left out
    teeth({"pooled": out}, o32, o64, o64_cut, f"GCNII's mean pool at H={H}")


def test_all_layers_of_a_forward_share_one_relation(monkeypatch):
    from graph_hscn.train import batching
    pm = _product_model("graph", False, "linear")
    bd = batching.to_device(pm, _model_batch(0, "linear", "graph"), DEV)
    spy = _CallSpy(monkeypatch)
    pm(bd).sum().backward()
    assert spy.names.count("hscn_gcn2_fwd") == M_L == spy.names.count("hscn_gcn2_bwd")
    assert spy.names.count("hscn_gcn_dinv") == 1 and spy.names.count("hscn_csr_build_pair") == 1


# --------------------------------------------------------------------------- #
# training, and the entry points that do not take the model
# --------------------------------------------------------------------------- #
def _peptides(count=8):
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    rng, edge_rng = np.random.default_rng(5), np.random.default_rng(6)
    return [make_graph(rng, SHAPES["peptides_func"], n=n, edge_features=True, edge_rng=edge_rng)
            for n in (1, 2, 7, 40, 23, 12, 31, 5)[:count]]


def test_one_epoch_of_train_runs_with_a_finite_loss_and_clean_flags():
    from graph_hscn.metrics import eval_ap
    from graph_hscn.train.train import train
    torch.manual_seed(3)
    pe = RWSEConfig(dim_in=9, dim_emb=16, dim_pe=4, ksteps=8)
    m = GCNII(9, 16, 10, 3, ACT_DICT["relu"], 0.1, 0.1, 0.5, False, True, "graph", "atom", pe).to(DEV)
    m.dropout_seed = 5
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    graphs = _peptides()
    cfg = SimpleNamespace(model_type="gcnii", epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10,
                          min_delta=0.0, metric="ap")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    history = train(None, opt, cfg, [DataLoader(graphs, 4), DataLoader(graphs, 8)], m, metric_fn=eval_ap)
    torch.cuda.synchronize()
    assert len(history) == 1 and np.isfinite(history[0][0]) and 0.0 <= history[0][1] <= 1.0     # (loss, the metric)
    m.check_flags()
    for k in ("layers.0.weight1", "layers.2.weight2", "node_encoder.weight", "pe_encoder.pe_encoder.0.weight"):
        assert not torch.equal(before[k], m.state_dict()[k]), k                # the step reached them


def test_the_resident_entry_points_refuse_the_model_with_its_own_reason():
    from graph_hscn.replay import CapturedStep
    from graph_hscn.train import batching
    from graph_hscn.train.train_resident import fit_resident
    m = GCNII(9, 16, 10, 2, ACT_DICT["relu"], node_encoder="atom").to(DEV)
    graphs = _peptides(4)
    bd = batching.to_device(m, Batch.from_data_list(graphs), DEV)
    with pytest.raises(RuntimeError, match=re.escape(m.resident_reason())):
        CapturedStep(m, SimpleNamespace(batch=bd), "cross_entropy")
    cfg = SimpleNamespace(model_type="gcnii", epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10,
                          min_delta=0.0, metric="ap")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match=re.escape(m.resident_reason())):
        fit_resident(None, opt, cfg, graphs, None, m, 4)
    m.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="GCNII's layers"):
        m(bd)
