"""The criteria of tests/test_gpu_f16_edges.py shown on the REFERENCE alone (no device, no launch).  A float32 stand-in
for the launches -- the CPU oracle in float32 with the kernels' rounding points, ``emulate_step`` -- is put through the
very functions the GPU tests call (``check_forward`` / ``check_virtual`` / ``check_gradients`` / ``check_stage_a``):

  * it passes the window criterion in every configuration and size class, and the conditions asserted on the windows
    (determined share >= 0.85, share wider than two halves <= 0.05, at s = 2^-12 a subnormal share >= 0.05 per layer)
    hold for it: they were chosen for the float32 oracle alone;
  * the forced float64 oracle satisfies ``KinkGuard.check(1e-5, 1e-5)`` at the committed seeds, and the stand-in's
    prediction, loss and gradients pass ``referee_all`` and its teeth;
  * three mutants of the stand-in are REJECTED here: a conversion that truncates, half subnormals flushed to zero on
    store, and a backward that differentiates the unrounded activation (the float32 oracle with rounding of the inputs
    only, exporting the rounded activations it never used).  On the inputs of tests/test_gpu_f16.py (the synthetic
    datasets' integer features; its bars restated in ``old_bars``, against the unmutated emulating oracle) the last two
    pass every bar of that file -- the flush changes nothing there at all -- and the truncation passes at L = 2 and is
    seen at L = 3 by the prediction bar alone.

If a case does not pass here, the seed or the case changes, never the bar.
"""
import numpy as np
import pytest
import torch

from oracle import models as OM
from tests import test_gpu_f16_edges as E
from tests.helpers import to_half

U, HALF_ULP = 2.0 ** -11, 2.0 ** -10


# --------------------------------------------------------------------------- #
# narrowing: the correct one and two wrong ones
# --------------------------------------------------------------------------- #
def truncating(t):
    """float -> half toward zero."""
    a = t.detach().cpu().numpy()
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
        over = np.abs(h.astype(a.dtype)) > np.abs(a)
        h[over] = np.nextafter(h[over], np.float16(0))
    return torch.from_numpy(h)


def flushing(t):
    """float -> half, round to nearest, results below the smallest normal flushed to zero."""
    h = to_half(t)
    h[h.abs() < 2.0 ** -14] = 0.0
    return h


class Rounding:
    """A tagged ``store``: narrows with ``narrow`` and records what it stored; ``layers``: which layer outputs round
    (None: all; (): the inputs only -- the activations it WOULD have stored are still recorded)."""
    tagged = True

    def __init__(self, narrow, layers=None):
        self.narrow, self.layers, self.stored = narrow, layers, {}

    def __call__(self, t, name, layer):
        h = self.narrow(t)
        self.stored[(name, layer)] = h
        if layer >= 0 and self.layers is not None and layer not in self.layers:
            return t
        return t + (h.to(t.dtype) - t).detach()


def emulate_step(om, ob, y, loss, narrow=to_half, unrounded_backward=False):
    """What ``test_gpu_f16_edges.run_step`` returns, from the float32 oracle with the kernels' rounding points."""
    B, L = int(ob["batch_local"].max()) + 1, len(om.convs)
    wrapped = E.OForced(om, loss)
    wrapped.store = Rounding(narrow, () if unrounded_backward else None)
    wrapped.zero_grad(set_to_none=True)
    pred, lossv = wrapped(ob["x_dict"], ob["edge_index_dict"], ob["batch_local"], B, y)
    lossv.backward()
    st = wrapped.store.stored
    grads = {"p.m." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in om.named_parameters()}
    om.zero_grad(set_to_none=True)
    return dict(acts=torch.stack([st[("local", l)] for l in range(L)]), virtual=st[("virtual", L - 1)],
                state0=st[("virtual", 0)], pred=pred.detach(), loss=lossv.detach(), grads=grads, defer=L >= 2,
                one_launch=False, exported=list(range(L)))


def old_bars(mut, ref, om, ob, L):
    """The assertions of tests/test_gpu_f16.py::test_half_storage_step_matches_the_emulating_oracle, restated: ``ref``
    is the emulating oracle (the unmutated stand-in).  Returns the list of bars ``mut`` misses."""
    B = int(ob["batch_local"].max()) + 1
    with torch.no_grad():
        plain = om(ob["x_dict"], ob["edge_index_dict"], ob["batch_local"], B)
    md = lambda a, b: float((a.double() - b.double()).abs().max())
    ps, vs = max(1.0, float(ref["pred"].abs().max())), max(1.0, float(ref["virtual"].float().abs().max()))
    gain = sum(2.0 ** l for l in range(1, L + 1))
    missed = []
    if md(mut["pred"], ref["pred"]) > HALF_ULP * ps:
        missed.append("pred")
    if md(mut["pred"], plain) > U * gain * ps:
        missed.append("pred vs plain float32")
    if md(mut["virtual"].float(), ref["virtual"].float()) > 2 * HALF_ULP * vs:
        missed.append("virtual")
    if abs(float(mut["loss"]) - float(ref["loss"])) > HALF_ULP * max(1.0, abs(float(ref["loss"]))):
        missed.append("loss")
    for k, g in ref["grads"].items():
        if g is not None and md(mut["grads"][k], g) > 4 * HALF_ULP * max(1e-3, float(g.abs().max())):
            missed.append(k)
    return missed


# --------------------------------------------------------------------------- #
# the float32 oracle alone meets the windows and their conditions
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("cls", list(E.SIZES))
@pytest.mark.parametrize("cfg", list(E.CONFIGS))
def test_the_float32_stand_in_meets_the_windows_and_their_conditions(cfg, cls):
    H, F, scale, ob, pb, spans, om = E.forward_case(cfg, cls)
    sub = scale < 1e-3
    what = f"stand-in {cfg} {cls}"
    maxima, plan = E.plan_of(pb, F, H, E.FWD_L)
    print(f"[f16 edges, host] {what}: maxima = {maxima} plan = {plan}")
    assert plan is not None and plan["threads"] == E.THREADS[cls]
    y = E.targets("l1", len(spans), E.FWD_SEED)
    dev = emulate_step(om, ob, y, "l1")
    E.check_forward(what, om, ob, spans, dev, E.FWD_L, subnormals=sub)
    om1, om2 = E.forward_case(cfg, cls, 1)[-1], E.forward_case(cfg, cls, 2)[-1]
    d1 = emulate_step(om1, ob, y, "l1")
    E.check_virtual(f"{what} virtual L=1", om1, ob, d1["virtual"], ob["x_dict"], 0, subnormals=sub)
    d2 = emulate_step(om2, ob, y, "l1")
    E.check_virtual(f"{what} virtual L=2 layer 0", om2, ob, d2["state0"], ob["x_dict"], 0, subnormals=sub)
    E.check_virtual(f"{what} virtual L=2 final", om2, ob, d2["virtual"],
                    {"local": d2["acts"][0].float(), "virtual": d2["state0"].float()}, 1, subnormals=sub)


@pytest.mark.parametrize("c", E.GRAD_CASES)
def test_the_forced_oracle_is_away_from_its_kinks_and_takes_the_stand_in(c):
    H, F, ob, pb, spans, om, y = E._grad_case(c["id"])
    what = "stand-in forced " + c["id"]
    maxima, plan = E.plan_of(pb, F, H, c["L"])
    print(f"[f16 edges, host] {what}: maxima = {maxima} plan = {plan}")
    assert plan is not None and plan["threads"] == E.THREADS[c["cls"]]
    dev = emulate_step(om, ob, y, c["loss"])
    print(f"   worst ratio: {E.check_gradients(what, om, ob, spans, y, dev, c['act'], c['loss']):.3f}")


# --------------------------------------------------------------------------- #
# mutants
# --------------------------------------------------------------------------- #
def _rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError as e:
        return str(e).splitlines()[0][:160]
    return None


OLD_CASES = [("pcqm_contact", 9, 16, 16, 3, 1, "relu", "l1"), ("pcqm_contact", 9, 16, 32, 2, 10, "tanh", "cross_entropy"),
             ("peptides_func", 6, 16, 16, 3, 10, "relu", "cross_entropy")]


def old_inputs(name, B, K, H, L, C, act, loss):
    """The inputs of tests/test_gpu_f16.py::test_half_storage_step_matches_the_emulating_oracle for one of its cases
    (integer atom features of the synthetic datasets): (oracle, batch, targets)."""
    from tests.test_gpu_f16 import _batches
    ob, _, _ = _batches(name, B, K, seed=B + K)
    torch.manual_seed(B)
    om = OM.HSCN("GAT", "GCN", "GCN", OM.ACT[act], ob["x_dict"]["local"].size(1), H, C, L)
    with torch.no_grad():
        for n_, p in om.named_parameters():
            if n_.endswith("bias"):
                p.normal_(0, 0.1)
    y = torch.randn(B, C, generator=torch.Generator().manual_seed(2))
    return om, ob, (y > 0).float() if loss == "cross_entropy" else y


MUTANTS = {"truncation": dict(narrow=truncating), "flushed subnormals": dict(narrow=flushing),
           "unrounded backward": dict(unrounded_backward=True)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
@pytest.mark.parametrize("old", OLD_CASES, ids=lambda c: f"{c[0]}-H{c[3]}-L{c[4]}")
def test_the_mutants_pass_every_bar_of_the_workload_shaped_file_on_its_own_inputs(old, mutant):
    om, ob, y = old_inputs(*old)
    ref = emulate_step(om, ob, y, old[7])
    mut = emulate_step(om, ob, y, old[7], **MUTANTS[mutant])
    missed = old_bars(mut, ref, om, ob, old[4])
    changed = not torch.equal(mut["acts"], ref["acts"]) or any(
        g is not None and not torch.equal(g, mut["grads"][k]) for k, g in ref["grads"].items())
    print(f"[f16 edges, host] {mutant} on {old[0]} H={old[3]} L={old[4]}: differs from the emulating oracle: {changed}; "
          f"bars of test_gpu_f16.py missed: {missed}")
    if mutant == "truncation" and old[4] == 3:
        # three truncated layers: a bias of -2^-11 relative per layer reaches that file's prediction bar (2^-10 of the
        # scale) at L = 3 and misses it at L = 2; recorded, not asserted either way -- the window criterion rejects a
        # truncating store in EVERY layer, by a thousand elements (below)
        assert set(missed) <= {"pred"}
        return
    assert not missed, f"{mutant}: the old bars see it at {missed}"


@pytest.mark.parametrize("cfg,mutant", [("H16-F9-s1", "truncation"), ("H32-F16-s1", "truncation"),
                                        ("H16-F3-s64", "truncation"), ("H16-F9-sub", "flushed subnormals")])
def test_conversion_mutants_are_rejected_by_the_window(cfg, mutant):
    H, F, scale, ob, pb, spans, om = E.forward_case(cfg, "t1024")
    y = E.targets("l1", len(spans), E.FWD_SEED)
    mut = emulate_step(om, ob, y, "l1", **MUTANTS[mutant])
    why = _rejected(E.check_forward, f"{mutant} {cfg}", om, ob, spans, mut, E.FWD_L, caps=False)
    print(f"[f16 edges, host] {mutant} at {cfg} rejected by the window criterion: {why}")
    assert why is not None and "outside the window" in why


# (one layer: the only stored activation feeds the pool alone, there is no backward through a stored activation)
@pytest.mark.parametrize("c", [p for p in E.GRAD_CASES if p.values[0]["L"] > 1])
def test_a_backward_on_the_unrounded_activation_is_rejected_under_forcing(c):
    H, F, ob, pb, spans, om, y = E._grad_case(c["id"])
    mut = emulate_step(om, ob, y, c["loss"], unrounded_backward=True)
    why = _rejected(E.check_gradients, "unrounded backward " + c["id"], om, ob, spans, y, mut, c["act"], c["loss"])
    print(f"[f16 edges, host] unrounded backward at {c['id']} rejected under forcing: {why}")
    assert why is not None and "outside the float64 referee" in why


# --------------------------------------------------------------------------- #
# stage A
# --------------------------------------------------------------------------- #
def emulate_stage_a(om, graphs, act, narrow=to_half, unrounded_backward=False):
    ys, Ss, mc, o = [], [], 0.0, 0.0
    om.zero_grad(set_to_none=True)
    for x, ei in graphs:
        with torch.no_grad():
            ys.append(narrow(E.scn_hidden(om, x, ei)[0]))
        if unrounded_backward:          # the stored value forward, act'(unrounded pre-activation) backward
            h, ei2 = E.scn_hidden(om, x, ei)
            h = h + (ys[-1].float() - h).detach()
        else:
            h, ei2 = E.scn_forced_hidden(om, act, x, ei, ys[-1].float())
        s = om._run_mlp(h)
        _, _, a, b = E.P.dense_mincut_pool(h, E.P.to_dense_adj(ei2), s)
        Ss.append(torch.softmax(s, dim=-1).detach())
        mc, o = mc + a, o + b
    ((mc + o) / len(graphs)).backward()
    out = {"p.m." + n: p.grad.detach().clone() for n, p in om.named_parameters()}
    om.zero_grad(set_to_none=True)
    out.update(y=torch.cat(ys), S=torch.cat(Ss), mc=(mc / len(graphs)).detach(), o=(o / len(graphs)).detach())
    return out


@pytest.mark.parametrize("id", list(E.SCN_CASES))
def test_stage_a_stand_in_and_its_truncating_mutant(id):
    H, act, F, Ka, graphs, om = E.scn_case(id)
    what = "stand-in stage A " + id
    print(f"[f16 edges, host] {what}")
    dev = emulate_stage_a(om, graphs, act)
    print(f"   worst ratio: {E.check_stage_a(what, om, graphs, act, F, dev, dev['y']):.3f}")
    mut = emulate_stage_a(om, graphs, act, truncating)
    why = _rejected(E.check_stage_a, what + " truncating", om, graphs, act, F, mut, mut["y"])
    print(f"   truncating mutant rejected: {why}")
    assert why is not None and "outside the window" in why
    if act != "relu":                   # (a ReLU's derivative is its gate: rounded or not, the same backward)
        mut = emulate_stage_a(om, graphs, act, unrounded_backward=True)
        why = _rejected(E.check_stage_a, what + " unrounded backward", om, graphs, act, F, mut, mut["y"])
        print(f"   unrounded-backward mutant rejected: {why}")
        assert why is not None and "outside the float64 referee" in why


def test_edge_biases_sit_where_they_are_named():
    b = E.edge_biases(32)
    assert b.numel() == 32 and E.edge_biases(16).numel() == 16
    h = b.half().float()
    assert float(h[0]) == 1.0 and float(h[1]) == 1.0 + 2.0 ** -9          # ties to even: down, then up
    assert float(h[2]) == 1.0 and float(h[3]) == 1.0 + 2.0 ** -10
    assert float(h[8]) == 0.0 and float(h[9]) == 0.0 and float(h[10]) == 2.0 ** -24      # the underflow tie
    assert float(h[11]) == 2.0 ** -23 and float(h[12]) == 2.0 ** -23                     # subnormal ties: up, then down
    assert float(h[13]) == 65504.0 and float(h[14]) == 65504.0 and torch.isinf(torch.tensor(65520.0).half())
    assert bool((to_half(b.double()) == b.half()).all())
