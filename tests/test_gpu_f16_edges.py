"""Half-precision STORAGE (``HSCN_STORE_F16``: csrc/resident_f16.hip, resident_kernels.h, resident_step.h,
resident_scn.hip; the helpers ``ldf4`` / ``stf4`` / ``stf_sc1`` / ``ldf4_sc1`` / ``rnd`` of resident_common.h) against
float64, at the rounding edges of IEEE half and at the size edges of the kernels: non-integer half features with full
mantissas, half subnormals, values next to 65504, the 4-wave / 16-wave workgroup class (64 / 65 nodes), the tails of
the 16-row tiles (1, 15, 16, 17 nodes), odd F.

tests/test_gpu_f16.py holds the same kernels to 2^-10 max|tensor| (gradients: 4 x that) on integer features: honest
bars -- a rounding-boundary flip between two float32 evaluations moves a stored value by one half ulp, and the next
layer carries it on -- but blind below 2^-11 relative.  Here the flip cannot propagate, because the launches export
what they stored and the oracle is FORCED onto it:

  * a stored tensor (``ResidentTrainStep.acts`` [L, N, H], ``.virtual``, the deferred state's virtual layer-0 output,
    ``ScnTrainStep.y``) is checked by the WINDOW criterion, ``helpers.half_window``: with r the float64 oracle's value of
    that layer from the device's own stored inputs (widened exactly), o32 the float32 oracle's from the same inputs and
    b = 2 max|o32 - r| + 8 * 2^-23 max|r| -- ``helpers.referee``'s bar, unchanged, per tensor -- half rounding is
    monotone, so a correct store d satisfies half(r - b) <= d <= half(r + b) element by element (both ends rounded
    once from the double); where the two ends are one half, d is determined to the bit; where the window holds an
    infinity or a NaN the device's pattern must match it;
  * ``pred``, the loss and every parameter gradient go through ``helpers.referee_all`` / ``teeth`` / ``KinkGuard`` as in
    tests/test_gpu_resident_f64.py, against the float32 and float64 oracle evaluated with ``helpers.ForcedStore``: every
    local activation replaced by the device's stored one (straight-through gradient), so all three backward passes read
    identical activations.  The guard's zone (4 x (1e-5 + 1e-5 |v|)) also covers a positive pre-activation below 2^-25
    that half stores as zero;
  * stage A (``k_scn_fwd`` / ``k_scn_bwd`` / ``k_scn_step``, one 1024-thread class: graphs of 1, 15, 16, 17, 57 and 64
    nodes) alike on ``y``, with one difference that the contract itself makes: the backward launch has the stored output
    only and evaluates act'(pre-activation) from it (``act_grad_from_output``), so the forced oracle does too
    (``scn_forced_hidden``).  For a ReLU that is the straight-through gate; for ELU the derivative at the rounded output
    is up to 2^-11 relative away from the one at the unrounded pre-activation -- a straight-through oracle is rejected
    at ratio 30 by the launches and, in turn, a backward on the unrounded activation by this one;
  * a node without in-edges gets relu(b_ll) exactly and stage A on zero features act(b_rel): biases at half rounding
    edges must come out as ``relu(b).half()`` bit for bit (b = 0 in the window: no tolerance at all).

No tolerance here is new and none is measured from the code under test.  The conditions asserted on the windows --
the share of positive elements determined to the bit >= 0.85, the share spanning more than two halves <= 0.05, at
s = 2^-12 a subnormal share >= 0.05 in every layer -- were chosen on the CPU so that the float32 oracle alone meets
them; tests/test_f16_edges_host.py asserts that without a GPU, with a float32 stand-in for the device, and shows three
mutants of it (truncating conversion, half subnormals flushed on store, a backward that differentiates the unrounded
activation) rejected here, the last two after passing every bar of tests/test_gpu_f16.py on that file's inputs.

Documented behaviour tested as documented: a value beyond 65519.99 stores as +inf (no
saturation), in the layer where it arises; every other graph of the batch is untouched bit for bit.  The kernels' ReLU
is ``fmaxf(v, 0)``, which returns zero for a NaN: behind an infinity the graph's later layers hold zeros where the oracle
holds NaN, and its prediction can be finite -- the infinity in ``acts`` is the record of the overflow.  The sign of a
zero that a ReLU produces is not specified (max(-0, +0)): zeros are compared as zeros.

The one-launch step (``hscn_resident_train_step<half_t>``) exports a_1 .. a_{L-1} -- not the last layer -- and only when
its virtual workgroups ride on idle CUs: its exported layers are held to the window criterion; where they are
``torch.equal`` to the pair's, prediction, loss and gradients are compared with the pair as tests/test_gpu_f16.py does
(``pool_order_close`` / ``grads_close``: the last layer is pooled out of the accumulators in another order), else under
that file's 2^-10 bars.  Stage A's one-launch form exports no ``y``: where its S is ``torch.equal`` to the pair's it is
held to the pair's forced oracle, else to the 2^-10 bar.  Each test prints which path ran.

Each case prints its window shares and referee lines; profiles/f16_edges_referee.txt records one run.  Nothing is
asserted from that file.
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F_

from oracle import hetero_data as OH
from oracle import models as OM
from oracle import pyg_ops as P
from tests.helpers import (DEV, ForcedStore, grads_close, half_window, in_half_window, most_changed, oracle_twin,
                           pool_order_close, referee, referee_all, relabel_graphs, teeth, to_half, window_shares)
from tests.test_gpu_layered_f64 import _drop_edges, _scn_gates
from tests.test_gpu_resident_f64 import LL, _LocalOut, _graph, named_edges, tree
from tests.test_gpu_scn_resident_f64 import YARDSTICK_SEEDS

pytestmark = pytest.mark.gpu

LV, VV = ("local", "to", "virtual"), ("virtual", "to", "virtual")
LLK = "local__to__local"
K, C = 8, 3
HALF_ULP = 2.0 ** -10                 # tests/test_gpu_f16.py's bar, where this file falls back to it
DETERMINED_MIN, WIDE_MAX, SUBNORMAL_MIN = 0.85, 0.05, 0.05

# (H, F, scale of the features): full mantissas at 1, half subnormals at 2^-12, the top of the half range at 64
CONFIGS = {"H16-F9-s1": (16, 9, 1.0), "H32-F16-s1": (32, 16, 1.0), "H16-F9-sub": (16, 9, 2.0 ** -12),
           "H16-F3-s64": (16, 3, 64.0)}
# nodes per graph: the 16-row tile tails; the 4-wave class takes graphs up to 64 nodes, the 16-wave class the rest
SIZES = {"t256": (1, 15, 16, 17, 64), "t1024": (1, 15, 16, 17, 64, 65, 70)}
THREADS = {"t256": 256, "t1024": 1024}


# --------------------------------------------------------------------------- #
# batches and models (no device)
# --------------------------------------------------------------------------- #
def build_batch(graphs, F, seed, scale):
    """``tests/test_gpu_resident_f64.build_batch`` with non-integer half features: x = (randn * scale).half(), widened.
    -> (oracle batch dict with half-representable features, product HeteroBatch on the CPU, [(offset, n)])."""
    from graph_hscn.data import Data, HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    data, ids = [], []
    for i, spec in enumerate(graphs):
        n = spec[1]
        ei, cid = _graph(spec, seed + 17 * i)
        x = (torch.randn(n, F, generator=g) * scale).half().float()
        data.append(Data(x=x, edge_index=ei, y=torch.zeros(1, C), num_nodes=n))
        ids.append(rng.integers(0, K, n) if cid is None else cid)
    ob = OH.collate_hetero([OH.hetero_from_clusters(d.x, d.edge_index, d.y, i, K) for d, i in zip(data, ids)])
    ob["x_dict"] = {k: to_half(v).float() for k, v in ob["x_dict"].items()}     # what the device widens
    pb = HeteroBatch.from_data_list([hetero_from_clusters(d, i, K) for d, i in zip(data, ids)])
    off = np.concatenate([[0], np.cumsum([s[1] for s in graphs])])
    return ob, pb, [(int(off[i]), s[1]) for i, s in enumerate(graphs)]


def oracle_model(F, H, L, act, seed, scale):
    """``OM.HSCN("GAT", "GCN", "GCN")`` with biases N(0, 0.1 min(scale, 1)): small features keep small activations."""
    torch.manual_seed(seed)
    om = OM.HSCN("GAT", "GCN", "GCN", OM.ACT[act], F, H, C, L)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p in om.named_parameters():
            if n_.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 * min(scale, 1.0))
    return om


def product_model(om, F, H, L, act):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    pm = HSCN("GAT", "GCN", "GCN", ACT_DICT[act], F, H, C, L).to(DEV)
    pm.load_state_dict(om.state_dict())
    pm.engine = "resident"
    return pm


def plan_of(pb, F, H, L):
    from graph_hscn import _hip
    maxima = (int(pb["local"].max_nodes), int(pb["virtual"].max_nodes), int(pb[LL].max_edges),
              int(pb[VV].max_edges))
    return maxima, _hip.resident_launch_plan(F, H, L, C, *maxima, True)


def targets(loss, B, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return (torch.rand(B, C, generator=g) > 0.5).float() if loss == "cross_entropy" else torch.randn(B, C, generator=g)


# --------------------------------------------------------------------------- #
# the device side: one step of the launch pair (or the one-launch step) and everything it exports, on the CPU
# --------------------------------------------------------------------------- #
def run_step(pm, pbd, loss, y, overlap, one_launch=False):
    from graph_hscn.step import ResidentTrainStep
    pm.overlap_virtual = overlap
    rs = ResidentTrainStep(pm, pbd, loss, target=y.to(DEV), one_launch=one_launch)
    rs.acts.zero_()
    rs.bind_grads()
    rs.run()
    torch.cuda.synchronize()
    rs.check()
    assert rs.acts.dtype == torch.float16 and rs.virtual.dtype == torch.float16
    names = {id(p): n for n, p in pm.named_parameters()}
    grads = {"p.m." + n: None for n, _ in pm.named_parameters()}
    grads.update({"p.m." + names[id(p)]: g.detach().cpu().clone() for p, g in rs.param_grads})
    V = pbd["virtual"].x.size(0)
    L = rs.dims[4]
    with_v = bool(rs.one_launch and rs.idle_cus and rs.virtual is not None)
    return dict(acts=rs.acts.cpu().clone(), virtual=rs.virtual[:V].cpu().clone(), pred=rs.pred.cpu().clone(),
                loss=rs.loss.cpu().clone(), grads=grads, partials=rs.partials.cpu().clone(),
                state0=rs._state[5].cpu().clone() if rs._state is not None else None, defer=bool(rs.defer),
                one_launch=bool(rs.one_launch),
                exported=list(range(L)) if not rs.one_launch else (list(range(L - 1)) if with_v and L >= 2 else []))


# --------------------------------------------------------------------------- #
# the window criterion
# --------------------------------------------------------------------------- #
def check_window(what, d, r64, o32, caps=True, subnormals=False):
    """Stored halves ``d`` against the window of (r64, o32); prints and (``caps``) asserts the shares.
    Returns (lo, hi, b)."""
    lo, hi, b = half_window(r64, o32)
    ok = in_half_window(d, lo, hi)
    sh = window_shares(r64, lo, hi, b)
    print(f"   window {what:44s} b = {b:.3e}  max|f64| = {float(r64.abs().max()) if r64.numel() else 0.0:.4g}  "
          f"outside = {int((~ok).sum())} of {ok.numel()}  determined = {sh['determined']:.3f}  "
          f"wide = {sh['wide']:.4f}  subnormal = {sh['subnormal']:.3f}  (of {sh['positive']} positive)")
    if not bool(ok.all()):
        k = int(torch.nonzero(~ok.flatten())[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} stored halves outside the window, first at {k}: stored "
                             f"{float(d.flatten()[k])!r}, window [{float(lo.flatten()[k])!r}, {float(hi.flatten()[k])!r}], "
                             f"f64 {float(r64.flatten()[k])!r}")
    if caps and sh["positive"]:
        assert sh["determined"] >= DETERMINED_MIN, f"{what}: only {sh['determined']:.3f} of the window is sharp"
        assert sh["wide"] <= WIDE_MAX, f"{what}: {sh['wide']:.3f} of the windows span more than two halves"
    if subnormals:
        assert sh["subnormal"] >= SUBNORMAL_MIN, f"{what}: {sh['subnormal']:.3f} half subnormals, the case is named for them"
    return lo, hi, b


def window_teeth(what, d, r64, o32, q64):
    """``q64``: the float64 value with one term removed.  Against ITS window (the float32 oracle's own distance kept)
    at least one element that window determines to the bit must be rejected."""
    lo, hi, _ = half_window(q64, o32.double() - r64 + q64)
    out = ~in_half_window(d, lo, hi) & (lo == hi)
    print(f"   window {what:44s} [one edge dropped] determined elements rejected: {int(out.sum())}")
    assert bool(out.any()), f"{what}: the window cannot see a dropped edge"


def _ll(m, l, x, ei):
    return m.convs[l].convs[LLK](x, ei).relu()


def _layer(m, l, xd, eis):
    return {k: v.relu() for k, v in m.convs[l](xd, eis).items()}


def check_forward(what, om, ob, spans, dev, L, caps=True, subnormals=False, layers=None):
    """Every exported local layer of ``dev`` by the window criterion (its input: the features, or the device's own
    stored layer before it), with the teeth of the two named edges.  ``layers``: the exported ones (default all)."""
    o64 = copy.deepcopy(om).double()
    eis = ob["edge_index_dict"]
    ei = eis[LL]
    named = named_edges(ei, spans)
    acts = dev["acts"]
    with torch.no_grad():
        for l in (range(L) if layers is None else layers):
            xin = ob["x_dict"]["local"] if l == 0 else acts[l - 1].float()
            r64, o32 = _ll(o64, l, xin.double(), ei), _ll(om, l, xin, ei)
            check_window(f"{what} acts[{l}]", acts[l], r64, o32, caps, subnormals)
            for e in named:
                keep = torch.ones(ei.size(1), dtype=torch.bool)
                keep[e] = False
                window_teeth(f"{what} acts[{l}]", acts[l], r64, o32, _ll(o64, l, xin.double(), ei[:, keep]))


def check_virtual(what, om, ob, d, xin, l, caps=True, subnormals=False):
    """Stored virtual features ``d`` of layer ``l`` from the inputs ``xin`` = {"local", "virtual"} (float32, widened)."""
    o64 = copy.deepcopy(om).double()
    eis = ob["edge_index_dict"]
    with torch.no_grad():
        r64 = _layer(o64, l, {k: v.double() for k, v in xin.items()}, eis)["virtual"]
        o32 = _layer(om, l, xin, eis)["virtual"]
    check_window(what, d, r64, o32, caps, subnormals)


# --------------------------------------------------------------------------- #
# gradients under forcing
# --------------------------------------------------------------------------- #
class OForced(nn.Module):
    """The oracle with its local activations forced (``store``: a ``ForcedStore``) -> prediction and criterion."""

    def __init__(self, m, loss):
        super().__init__()
        self.m, self.loss, self.l1_gate, self.store = m, loss, nn.Identity(), None

    def forward(self, xd, eis, batch_local, B, y):
        pred = self.m(xd, eis, batch_local, B, store=self.store)
        if self.loss == "l1":
            self.l1_gate(pred - y)
            return pred, F_.l1_loss(pred, y)
        return pred, F_.binary_cross_entropy_with_logits(pred, y, reduction="mean")


def _gates(act, loss):
    def gates(m):
        g = [_LocalOut(c) for c in m.m.convs]
        if act == "relu":
            g.append(m.m.lin_1)
        if loss == "l1":
            g.append(m.l1_gate)
        return g
    return gates


def forced_eval(om, ob, y, dtype, eis=None, gates=None):
    """{"pred", "loss", "p.m.<parameter>"} of the forced oracle ``om`` in ``dtype``, and the kink guard."""
    keep = {}
    B = int(ob["batch_local"].max()) + 1

    def step(m, dt):
        m.store = om.store
        pred, loss = m({k: v.to(dt) for k, v in ob["x_dict"].items()}, eis if eis is not None else ob["edge_index_dict"],
                       ob["batch_local"], B, y.to(dt))
        loss.backward()
        keep.update(pred=pred.detach(), loss=loss.detach())

    grads, kg, _ = oracle_twin(om, step, dtype, gates, guard=gates is not None)
    return dict(grads, **keep), kg


def check_gradients(what, om, ob, spans, y, dev, act, loss):
    """``dev``'s prediction, loss and parameter gradients against the oracle forced onto ``dev``'s stored activations:
    kink guard on the float64 one, ``referee_all``, ``teeth`` with dropped local -> local edges.  Returns the worst
    ratio."""
    L = dev["acts"].size(0)
    wrapped = OForced(om, loss)
    wrapped.store = ForcedStore({("local", l): dev["acts"][l].float() for l in range(L)})
    o32, _ = forced_eval(wrapped, ob, y, torch.float32)
    o64, kg = forced_eval(wrapped, ob, y, torch.float64, gates=_gates(act, loss))
    kg.check(1e-5, 1e-5, what)
    got = dict(dev["grads"], pred=dev["pred"], loss=dev["loss"])
    worst = referee_all(got, o32, o64, what)
    ei = ob["edge_index_dict"][LL]
    dropped = [forced_eval(wrapped, ob, y, torch.float64, eis={**ob["edge_index_dict"], LL: e})[0]
               for (e,) in _drop_edges(ei, must=named_edges(ei, spans))]
    reached = most_changed(o64, dropped)
    assert reached, f"{what}: the dropped edge reaches no gradient"
    print(f"   teeth: one dropped edge reaches {sorted(reached)}")
    teeth(got, o32, o64, reached, what)
    return worst


# --------------------------------------------------------------------------- #
# 1. known answers for the conversion itself
# --------------------------------------------------------------------------- #
def edge_biases(H):
    """float32 values at the rounding edges of IEEE half, H of them (H = 16: the first 16; H = 32: all and negatives)."""
    up, dn = (lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))), \
             (lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf))))
    tie_even, tie_odd = 1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11
    v = [tie_even, tie_odd, dn(tie_even), up(tie_even), dn(tie_odd), up(tie_odd),            # ties, either side
         dn(2.0 ** -14), up(2.0 ** -14),                                                      # subnormal / normal border
         2.0 ** -25, dn(2.0 ** -25), up(2.0 ** -25),                                          # the underflow tie
         3.0 * 2.0 ** -25, 5.0 * 2.0 ** -25,                                                  # subnormal ties (even, odd)
         65504.0, 65519.99, -0.0,
         # H = 32
         -tie_even, -2.0 ** -25, -65520.0, 1023.0 * 2.0 ** -24 + 2.0 ** -25, dn(2.0 ** -14 - 2.0 ** -25),
         up(3.0 * 2.0 ** -25), dn(5.0 * 2.0 ** -25), 2.0 ** -24, up(2.0 ** -24), 0.333251953125 + 2.0 ** -13,
         2047.5, 2048.5 + 2.0 ** -10, 32767.99, 60000.03, dn(65504.0), up(65504.0)]
    return torch.tensor(v[:H], dtype=torch.float32)


def same_halves(a, b):
    """Bit for bit, zeros compared as zeros (the sign of relu's zero is unspecified)."""
    a, b = a.cpu().clone(), b.cpu().clone()
    a[a == 0], b[b == 0] = 0.0, 0.0
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def set_ll_biases(om, per_layer):
    with torch.no_grad():
        for l, b in enumerate(per_layer):
            om.convs[l].convs[LLK].bias.copy_(b)


def exact_case(H, overflow):
    """Graphs of isolated nodes; layer l's bias is the edge list rolled by l (every value in every column class of
    the 4-wide stores); ``overflow``: 65520 (-> inf) in the LAST layer's bias -- an infinity in an earlier layer
    would reach this one as inf * 0."""
    F, L, seed = 9, 3, 2
    graphs = [("empty", n) for n in (1, 15, 16, 17, 64, 65)]
    ob, pb, spans = build_batch(graphs, F, seed, 1.0)
    om = oracle_model(F, H, L, "relu", seed, 1.0)
    bs = [torch.roll(edge_biases(H), l) for l in range(L)]
    if overflow:
        bs[L - 1][1], bs[L - 1][6] = 65520.0, 7.0e4
    set_ll_biases(om, bs)
    return F, L, ob, pb, om, bs


@pytest.mark.parametrize("overflow", [False, True], ids=["finite", "overflow-in-last-layer"])
@pytest.mark.parametrize("H", [16, 32])
def test_isolated_nodes_store_relu_of_the_bias_exactly(H, overflow):
    F, L, ob, pb, om, bs = exact_case(H, overflow)
    pm = product_model(om, F, H, L, "relu")
    pbd = pb.to(DEV).with_feature_dtype(torch.float16)
    y = targets("l1", int(ob["batch_local"].max()) + 1, 0)
    N = ob["x_dict"]["local"].size(0)
    want = [b.relu().half().expand(N, H) for b in bs]
    assert overflow == bool(torch.isinf(want[L - 1]).any())
    for name, overlap, one in (("pair", False, False), ("pair with_virtual", True, False), ("one-launch", True, None)):
        dev = run_step(pm, pbd, "l1", y, overlap, one)
        print(f"[f16 edges] exact H={H} {name}: one_launch = {dev['one_launch']} defer = {dev['defer']} "
              f"exported layers = {dev['exported']}")
        for l in dev["exported"]:
            assert same_halves(dev["acts"][l], want[l]), f"{name}: acts[{l}] is not relu(b).half() bit for bit"
        if one is None and not dev["one_launch"]:
            print("   (the one-launch step does not take this batch here: the pair ran)")


@pytest.mark.parametrize("act", ["relu", "identity"])
@pytest.mark.parametrize("H", [16, 32])
def test_stage_a_on_zero_features_stores_act_of_the_bias_exactly(H, act):
    from graph_hscn.step import ScnTrainStep
    F, Ka, seed = 9, 4, 2
    graphs = [(torch.zeros(n, F), tree(n, seed + i)) for i, n in enumerate((1, 15, 16, 17, 57, 64))]
    torch.manual_seed(seed)
    om = OM.SCN([H], act, F, Ka)
    b = edge_biases(H)
    if act == "identity":
        b = torch.roll(b, 3)
    with torch.no_grad():
        om.mp.module_0.lin_rel.bias.copy_(b)
    pm, data = scn_product(om, graphs, H, act, F, Ka)
    st = ScnTrainStep(pm, data, one_launch=False)
    st.run()
    torch.cuda.synchronize()
    st.check()
    assert st.y.dtype == torch.float16
    want = OM.ACT[act](b).half().expand(data.x.size(0), H)
    assert same_halves(st.y, want), "y is not act(b_rel).half() bit for bit"


def test_an_overflowing_graph_leaves_the_other_graphs_untouched():
    """One graph's features are +-60000, signed like the widest row of layer 0's weight, so that its layer-0
    activations pass 65520 in that column and store as +inf (documented: no saturation), exactly where the window
    says.  Every other graph's stored activations, prediction and per-graph gradient partials equal, bit for bit,
    those of the same batch with that graph's features left small.  (The overflowing graph's own later layers are
    not compared: the kernels' ReLU is a max, so a NaN pre-activation -- inf * w sums -- stores as zero.)"""
    H, F, L, seed = 16, 9, 3, 4
    graphs = [("tree", n) for n in (15, 17, 33, 64)]
    ob, pb, spans = build_batch(graphs, F, seed, 1.0)
    om = oracle_model(F, H, L, "relu", seed, 1.0)
    pm = product_model(om, F, H, L, "relu")
    y = targets("l1", len(graphs), seed)
    o, n = spans[2]
    w = om.convs[0].convs[LLK].lin.weight.detach()
    big = pb.to(DEV)
    big["local"].x = big["local"].x.clone()
    big["local"].x[o:o + n] = (60000.0 * torch.sign(w[int(w.abs().sum(1).argmax())])).to(DEV)    # finite in half
    runs = [run_step(pm, b.with_feature_dtype(torch.float16), "l1", y, False) for b in (pb.to(DEV), big)]
    a0, a1 = runs[0]["acts"], runs[1]["acts"]
    assert bool(torch.isfinite(a0.float()).all()) and bool(torch.isinf(a1[0, o:o + n].float()).any())
    # layer 0 of the whole batch, infinities included: where half(r - b) is +inf the store must be +inf
    ob["x_dict"]["local"][o:o + n] = big["local"].x[o:o + n].cpu()
    o64 = copy.deepcopy(om).double()
    with torch.no_grad():
        r64 = _ll(o64, 0, ob["x_dict"]["local"].double(), ob["edge_index_dict"][LL])
        o32 = _ll(om, 0, ob["x_dict"]["local"], ob["edge_index_dict"][LL])
    lo, _, _ = check_window("overflow acts[0]", a1[0], r64, o32, caps=False)
    assert bool(torch.isinf(lo.float()).any()), "the window itself demands an infinity somewhere"
    print(f"   the overflowing graph's prediction: {runs[1]['pred'][2].tolist()} (a NaN pre-activation stores as zero)")
    others = torch.ones(a0.size(1), dtype=torch.bool)
    others[o:o + n] = False
    assert torch.equal(a0[:, others].view(torch.int16), a1[:, others].view(torch.int16))
    rows = [0, 1, 3]
    assert torch.equal(runs[0]["pred"][rows], runs[1]["pred"][rows])
    assert torch.equal(runs[0]["partials"][rows][:, :-1], runs[1]["partials"][rows][:, :-1]), \
        "the per-graph gradient partials of the other graphs"
    print("[f16 edges] overflow: graph 2 stores +inf, graphs 0, 1, 3 bit-identical in acts, pred and gradient partials")


# --------------------------------------------------------------------------- #
# 2. launch pair, forward windows
# --------------------------------------------------------------------------- #
FWD_SEED, FWD_L = 3, 3


@functools.lru_cache(maxsize=None)
def forward_case(cfg, cls, L=FWD_L):
    H, F, scale = CONFIGS[cfg]
    graphs = [("tree", n) for n in SIZES[cls]]
    ob, pb, spans = build_batch(graphs, F, FWD_SEED, scale)
    om = oracle_model(F, H, L, "relu", FWD_SEED, scale)
    return H, F, scale, ob, pb, spans, om


@pytest.mark.parametrize("cls", list(SIZES))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_pair_forward_windows(cfg, cls):
    H, F, scale, ob, pb, spans, om = forward_case(cfg, cls)
    what = f"pair {cfg} {cls}"
    maxima, plan = plan_of(pb, F, H, FWD_L)
    print(f"[f16 edges] {what}: maxima = {maxima} plan = {plan}")
    assert plan is not None and plan["threads"] == THREADS[cls]
    pm = product_model(om, F, H, FWD_L, "relu")
    dev = run_step(pm, pb.to(DEV).with_feature_dtype(torch.float16), "l1", targets("l1", len(spans), FWD_SEED), False)
    check_forward(what, om, ob, spans, dev, FWD_L, subnormals=scale < 1e-3)


@pytest.mark.parametrize("cls", list(SIZES))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_pair_virtual_windows(cfg, cls):
    """The final virtual features at L = 1 (``hscn_resident_fwd``, with ``overlap_virtual`` off and on: one layer is
    never deferred) and, at L = 2 on the deferred route, the state's layer-0 output from the features and the final
    features from that state and the device's ``acts[0]``.  Deeper virtual layers keep tests/test_gpu_f16.py's bar."""
    H, F, scale, ob, pb, spans, om1 = forward_case(cfg, cls, 1)
    sub = scale < 1e-3
    what = f"virtual {cfg} {cls}"
    print(f"[f16 edges] {what}")
    y = targets("l1", len(spans), FWD_SEED)
    pbd = pb.to(DEV).with_feature_dtype(torch.float16)
    pm = product_model(om1, F, H, 1, "relu")
    for overlap in (False, True):
        dev = run_step(pm, pbd, "l1", y, overlap)
        assert not dev["defer"]
        check_virtual(f"{what} L=1 overlap={overlap}", om1, ob, dev["virtual"], ob["x_dict"], 0, subnormals=sub)
    om2 = forward_case(cfg, cls, 2)[-1]
    pm = product_model(om2, F, H, 2, "relu")
    dev = run_step(pm, pbd, "l1", y, True)
    assert dev["defer"] and dev["state0"] is not None, "2 B <= CUs: the virtual branch rides on both launches"
    check_virtual(f"{what} L=2 deferred layer 0", om2, ob, dev["state0"], ob["x_dict"], 0, subnormals=sub)
    check_virtual(f"{what} L=2 deferred final", om2, ob, dev["virtual"],
                  {"local": dev["acts"][0].float(), "virtual": dev["state0"].float()}, 1, subnormals=sub)
    plain = run_step(pm, pbd, "l1", y, False)
    assert same_halves(plain["virtual"], dev["virtual"]) and torch.equal(plain["acts"], dev["acts"])
    # L = 3: the final virtual features under the existing bar
    H, F, scale, ob, pb, spans, om3 = forward_case(cfg, cls)
    pm = product_model(om3, F, H, FWD_L, "relu")
    dev = run_step(pm, pbd, "l1", y, True)
    keep = {}
    with torch.no_grad():
        om3(ob["x_dict"], ob["edge_index_dict"], ob["batch_local"], len(spans), store=OM.half_storage, keep=keep)
    vs = float(keep["virtual"].abs().max())
    dv = float((dev["virtual"].double() - keep["virtual"].double()).abs().max())
    print(f"   {what} L=3 final: |virtual - emulating oracle| = {dv:.3e}  bar = {2 * HALF_ULP * max(vs, 2.0 ** -14):.3e}")
    assert dv <= 2 * HALF_ULP * max(vs, 2.0 ** -14)


# --------------------------------------------------------------------------- #
# 3. launch pair, gradients under forcing (scale 1).  seeds: constants chosen on the CPU (tests/test_f16_edges_host.py)
# so that the forced float64 oracle satisfies KinkGuard.check(1e-5, 1e-5) with room to spare.
# --------------------------------------------------------------------------- #
def gcase(id, cfg, L, loss, cls, seed, act="relu"):
    return pytest.param(dict(id=id, cfg=cfg, L=L, loss=loss, cls=cls, seed=seed, act=act), id=id)


# L = 3 on fewer nodes: layers 1 and 2 are evaluated from the DEVICE's stored activations, and a rounding flip against
# the CPU stand-in the seeds were chosen with moves a neighbour's pre-activation by ~5e-5 -- those seeds keep every gate
# input six times the guard's distance from zero on the stand-in, which fewer elements make findable
GRAD_SIZES = {(1, "t256"): (1, 15, 16, 17, 64), (1, "t1024"): (15, 17, 64, 65, 70),
              (3, "t256"): (15, 17, 64), (3, "t1024"): (17, 65)}
GRAD_CASES = [
    gcase("H16-L1-l1-t256", "H16-F9-s1", 1, "l1", "t256", 1),
    gcase("H16-L1-ce-t1024", "H16-F9-s1", 1, "cross_entropy", "t1024", 4),
    gcase("H16-L3-l1-t1024", "H16-F9-s1", 3, "l1", "t1024", 6),
    gcase("H16-L3-ce-t256", "H16-F9-s1", 3, "cross_entropy", "t256", 13),
    gcase("H32-L1-l1-t1024", "H32-F16-s1", 1, "l1", "t1024", 1),
    gcase("H32-L1-ce-t256", "H32-F16-s1", 1, "cross_entropy", "t256", 1),
    gcase("H32-L3-l1-t256", "H32-F16-s1", 3, "l1", "t256", 189),
    gcase("H32-L3-ce-t1024", "H32-F16-s1", 3, "cross_entropy", "t1024", 6),
]


@functools.lru_cache(maxsize=None)
def _grad_case(id):
    c = next(p.values[0] for p in GRAD_CASES if p.values[0]["id"] == id)
    H, F, scale = CONFIGS[c["cfg"]]
    graphs = [("tree", n) for n in GRAD_SIZES[c["L"], c["cls"]]]
    ob, pb, spans = build_batch(graphs, F, c["seed"], scale)
    om = oracle_model(F, H, c["L"], c["act"], c["seed"], scale)
    return H, F, ob, pb, spans, om, targets(c["loss"], len(spans), c["seed"])


def same_step(a, b, what):
    assert torch.equal(a["pred"], b["pred"]) and torch.equal(a["loss"], b["loss"]), f"{what}: prediction or loss"
    assert torch.equal(a["acts"], b["acts"]), f"{what}: stored activations"
    for k, v in a["grads"].items():
        assert (v is None and b["grads"][k] is None) or torch.equal(v, b["grads"][k]), f"{what}: {k}"


@pytest.mark.parametrize("c", GRAD_CASES)
def test_pair_gradients_under_forcing(c):
    H, F, ob, pb, spans, om, y = _grad_case(c["id"])
    what = "forced " + c["id"]
    maxima, plan = plan_of(pb, F, H, c["L"])
    print(f"[f16 edges] {what}: maxima = {maxima} plan = {plan}")
    assert plan is not None and plan["threads"] == THREADS[c["cls"]]
    pm = product_model(om, F, H, c["L"], c["act"])
    pbd = pb.to(DEV).with_feature_dtype(torch.float16)
    dev = run_step(pm, pbd, c["loss"], y, False)
    print(f"   worst ratio: {check_gradients(what, om, ob, spans, y, dev, c['act'], c['loss']):.3f}")
    if c["id"] == "H16-L3-l1-t1024":
        # the _with_virtual launches, and the autograd route on a half batch: the pair's bits
        from graph_hscn.loss import criterion
        over = run_step(pm, pbd, c["loss"], y, True)
        assert over["defer"]
        same_step(over, dev, f"{what} with_virtual")
        pm.overlap_virtual = False
        pm.zero_grad(set_to_none=True)
        pred = pm(pbd.x_dict, pbd.edge_index_dict, pbd)
        loss, _ = criterion(c["loss"], pred, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        assert pm.last_engine == "resident" and torch.equal(pred.detach().cpu(), dev["pred"])
        assert torch.equal(loss.detach().cpu(), dev["loss"])
        for n_, p in pm.named_parameters():
            g = dev["grads"]["p.m." + n_]
            assert (p.grad is None and g is None) or torch.equal(p.grad.cpu(), g), f"{what} autograd: {n_}"
        print("   with_virtual launches and the autograd route: bit-identical to the pair")


# --------------------------------------------------------------------------- #
# 4. the one-launch step
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("id", ["H16-L3-l1-t1024", "H32-L3-l1-t256", "H16-L3-ce-t256"])
def test_one_launch_step(id):
    c = next(p.values[0] for p in GRAD_CASES if p.values[0]["id"] == id)
    H, F, ob, pb, spans, om, y = _grad_case(id)
    what = "one-launch " + id
    pm = product_model(om, F, H, c["L"], c["act"])
    pbd = pb.to(DEV).with_feature_dtype(torch.float16)
    pair = run_step(pm, pbd, c["loss"], y, False)
    one = run_step(pm, pbd, c["loss"], y, True, one_launch=None)
    print(f"[f16 edges] {what}: one_launch = {one['one_launch']} exported layers = {one['exported']}")
    if not one["one_launch"]:
        same_step(one, pair, what + " (resolved to the pair)")
        return
    check_forward(what, om, ob, spans, one, c["L"], layers=one["exported"])
    same = bool(one["exported"]) and all(torch.equal(one["acts"][l], pair["acts"][l]) for l in one["exported"])
    print(f"   exported layers bit-identical to the pair's: {same}")
    if same:
        assert pool_order_close(one["pred"], pair["pred"]) and pool_order_close(one["loss"], pair["loss"])
        for k, v in pair["grads"].items():
            assert (v is None and one["grads"][k] is None) or grads_close(one["grads"][k], v), k
    else:
        ps = max(1.0, float(pair["pred"].abs().max()))
        assert float((one["pred"] - pair["pred"]).abs().max()) <= HALF_ULP * ps
        for k, v in pair["grads"].items():
            if v is not None:
                assert float((one["grads"][k] - v).abs().max()) <= 4 * HALF_ULP * max(1e-3, float(v.abs().max())), k


# --------------------------------------------------------------------------- #
# 5. stage A
# --------------------------------------------------------------------------- #
SCN_SIZES = (1, 15, 16, 17, 57, 64)          # one workgroup class (1024 threads): the 16-row tile tails, F = 9 odd
SCN_CASES = {"H16-relu": (16, "relu", 9, 4, 1), "H32-elu": (32, "elu", 9, 8, 1)}      # H, act, F, K, seed


def scn_product(om, graphs, H, act, F, Ka):
    from graph_hscn.data import Batch, Data
    from graph_hscn.model.hscn import SCN
    pm = SCN([H], act, F, Ka).to(DEV)
    pm.load_state_dict(om.state_dict())
    data = Batch.from_data_list([Data(x=x, edge_index=ei, num_nodes=x.size(0)) for x, ei in graphs]).to(DEV)
    data.x = data.x.half()
    return pm, data


@functools.lru_cache(maxsize=None)
def scn_case(id):
    H, act, F, Ka, seed = SCN_CASES[id]
    g = torch.Generator().manual_seed(seed)
    graphs = [((torch.randn(n, F, generator=g)).half().float(), tree(n, seed + 17 * i)) for i, n in enumerate(SCN_SIZES)]
    torch.manual_seed(seed)
    return H, act, F, Ka, graphs, OM.SCN([H], act, F, Ka)


def scn_hidden(m, x, ei):
    """The hidden activation BEFORE storage in the dtype of ``m``: gcn_norm(add_self_loops=True) -> GraphConv -> act."""
    dt = m.mp.module_0.lin_rel.weight.dtype
    ei2, ew = P.gcn_norm(ei, None, x.size(0), add_self_loops=True, dtype=dt)
    return m.mp(x.to(dt), ei2, ew), ei2


def act_grad_from_output(y, act):
    """d act / d pre-activation written through the OUTPUT, as every kernel of the project evaluates it
    (hscn_common.h: act_grad_from_output) -- and the stored output is all the backward launch has."""
    if act == "relu":
        return (y > 0).to(y.dtype)
    if act == "elu":
        return torch.where(y > 0, torch.ones_like(y), y + 1.0)
    if act == "tanh":
        return 1.0 - y * y
    return torch.ones_like(y)


def scn_forced_hidden(m, act, x, ei, y):
    """The hidden activation FORCED onto the stored ``y``, with the gradient the backward launch's contract gives it
    (resident_common.h: forward and backward see one and the same rounded value): value y, derivative with respect to
    the pre-activation act'(y) from the stored output.  For a ReLU that is the straight-through ``t + (y - t).detach()``
    (the kink guard holds the gate); for ELU / tanh the derivative at the rounded output differs from the one at the
    unrounded pre-activation by up to 2^-11 relative, and only the former is what the kernel can compute."""
    dt = m.mp.module_0.lin_rel.weight.dtype
    ei2, ew = P.gcn_norm(ei, None, x.size(0), add_self_loops=True, dtype=dt)
    pre = m.mp.module_0(x.to(dt), ei2, ew)
    y = y.to(dt).detach()
    return y + act_grad_from_output(y, act) * (pre - pre.detach()), ei2


class OSCNForced(nn.Module):
    """The oracle's stage-A body per graph on [x | forced y] rows (one tensor, so that ``helpers.relabel_graphs``
    permutes both alike) -> [mean mc, mean o]; ``last_S``: the assignments of the last call."""

    def __init__(self, m, F, act):
        super().__init__()
        self.m, self.F, self.act = m, F, act

    def forward(self, graphs):
        mc, o, Ss = 0.0, 0.0, []
        for xy, ei in graphs:
            x, y = xy[:, :self.F], xy[:, self.F:]
            h, ei2 = scn_forced_hidden(self.m, self.act, x, ei, y)
            s = self.m._run_mlp(h)
            _, _, a, b = P.dense_mincut_pool(h, P.to_dense_adj(ei2).to(h.dtype), s)
            Ss.append(torch.softmax(s, dim=-1).detach())
            mc, o = mc + a, o + b
        self.last_S = torch.cat(Ss)
        return torch.stack([mc / len(graphs), o / len(graphs)])


def scn_forced_eval(wrapped, graphs, dtype, gates=None):
    keep = {}

    def step(m, dt):
        out = m([(xy.to(dt), ei) for xy, ei in graphs])
        out.sum().backward()
        keep.update(mc=out[0].detach(), o=out[1].detach(), S=m.last_S)

    grads, kg, _ = oracle_twin(wrapped, step, dtype, gates, guard=gates is not None)
    return dict(grads, **keep), kg


def check_stage_a(what, om, graphs, act, F, dev, y_forced, window=True):
    """``dev`` = {"y" (or None), "S", "mc", "o", "p.m.*"}: ``y`` by the window criterion, everything else by the referee
    against the oracle forced onto ``y_forced`` -- eight float32 draws (the batch and seven relabelled copies) for the
    losses and gradients, which no relabelling changes; S, whose rows follow the nodes, against the first."""
    o64m = copy.deepcopy(om).double()
    off = np.concatenate([[0], np.cumsum([x.size(0) for x, _ in graphs])])
    if window:
        with torch.no_grad():
            r64 = torch.cat([scn_hidden(o64m, x, ei)[0] for x, ei in graphs])
            o32 = torch.cat([scn_hidden(om, x, ei)[0] for x, ei in graphs])
        check_window(f"{what} y", dev["y"], r64, o32)
    forced = [(torch.cat([x, y_forced[off[i]:off[i + 1]].float()], 1), ei) for i, (x, ei) in enumerate(graphs)]
    wrapped = OSCNForced(om, F, act)
    o32s = [scn_forced_eval(wrapped, forced, torch.float32)[0]]
    o32s += [scn_forced_eval(wrapped, relabel_graphs(forced, s), torch.float32)[0] for s in YARDSTICK_SEEDS]
    o64, kg = scn_forced_eval(wrapped, forced, torch.float64, gates=_scn_gates(act))
    kg.check(1e-5, 1e-5, what)
    got = {k: v for k, v in dev.items() if k != "y"}
    assert referee(got.pop("S"), o32s[0].pop("S"), o64.pop("S"), f"{what} S") <= 1.0, f"{what}: S outside the referee"
    for d in o32s[1:]:
        d.pop("S")
    worst = referee_all(got, o32s, o64, what)
    big = max(range(len(graphs)), key=lambda i: graphs[i][0].size(0))
    n, ei = graphs[big][0].size(0), graphs[big][1]
    must = [int(torch.nonzero(ei[1] == node).flatten()[0]) for node in (n - 1, 16 * ((n - 1) // 16))]
    dropped = []
    for (e,) in _drop_edges(ei, must=must):
        d = scn_forced_eval(wrapped, [(xy, e if i == big else gei) for i, (xy, gei) in enumerate(forced)], torch.float64)[0]
        d.pop("S")
        dropped.append(d)
    reached = most_changed(o64, dropped)
    assert reached, f"{what}: the dropped edge reaches nothing"
    print(f"   teeth: one dropped edge reaches {sorted(reached)}")
    teeth(got, o32s, o64, reached, what)
    return worst


def _scn_out(pm, S, losses, grads, y=None):
    names = {id(p): n for n, p in pm.named_parameters()}
    out = {"p.m." + names[id(p)]: g.detach().cpu().clone() for p, g in grads}
    out.update(S=S.cpu().clone(), mc=losses[0].cpu().clone(), o=losses[1].cpu().clone(), y=None if y is None else y.cpu().clone())
    return out


@pytest.mark.parametrize("id", list(SCN_CASES))
def test_stage_a_under_forcing(id):
    from graph_hscn.step import ScnTrainStep
    H, act, F, Ka, graphs, om = scn_case(id)
    what = "stage A " + id
    print(f"[f16 edges] {what}")
    pm, data = scn_product(om, graphs, H, act, F, Ka)
    st = ScnTrainStep(pm, data, one_launch=False)
    st.run()
    torch.cuda.synchronize()
    st.check()
    assert st.y.dtype == torch.float16
    pair = _scn_out(pm, st.S, st.losses, st.param_grads, st.y)
    print(f"   worst ratio, launch pair: {check_stage_a(what + ' pair', om, graphs, act, F, pair, pair['y']):.3f}")
    one = ScnTrainStep(pm, data, one_launch=True)
    one.run()
    torch.cuda.synchronize()
    one.check()
    step = _scn_out(pm, one.S, one.losses, one.param_grads)
    same = torch.equal(step["S"], pair["S"])
    print(f"   one-launch step: S bit-identical to the pair's: {same}")
    if same:
        print(f"   worst ratio, one-launch step: "
              f"{check_stage_a(what + ' step', om, graphs, act, F, step, pair['y'], window=False):.3f}")
    else:
        assert float((step["S"] - pair["S"]).abs().max()) <= HALF_ULP
        for k, v in pair.items():
            if k.startswith("p."):
                assert float((step[k] - v).abs().max()) <= 4 * HALF_ULP * max(1e-3, float(v.abs().max())), k
