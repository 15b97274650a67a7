"""hscn_class_weights + hscn_softmax_nll_fwd_ex (csrc/loss.hip) against float64 ``F.cross_entropy(pred, true,
weight=w, ignore_index=i)`` on the CPU.

Bounds: ``tests/helpers.check_f64`` with ``F64_C`` as it is.  With u = 2^-24:
  * logp = (x - m) - log s, s = sum_c exp(x_c - m) >= 1.  exp(a) of a rounded argument carries a relative error
    (|a| + 2) u, and sum_c |a_c| exp(a_c) <= C / e, so with the C - 1 adds s is within (2 C + 4) u of its value
    relatively, which log turns into the same absolute error; the two subtractions and log's own rounding add u each
    of |x| + |m| + |log s|.  n = 2 C + 8, mag = |x| + |m| + |log s| + 1.
  * grad = w_y (p - onehot) / denom: p = exp(x - m) / s inherits s's relative error; the weight product, the
    subtraction, the rounding of the denominator and the division by it add one each.  n = 2 C + 12,
    mag = w_y (p + onehot) / denom.
  * loss = sum_r w_r (-logp_r) / denom: a sum of R terms, each with logp's error.  n = R + 2 C + 12,
    mag = sum_r w_r (|x| + |m| + |log s| + 1) / denom.
Each comes with a dropped-term reference the same bound must reject: the loss without the row of the largest
w |logp|, logp with the largest term missing from one row's sum, grad with one row's onehot missing.  C = 1 makes every
logp, term and gradient exactly zero -- nothing can be dropped from zero -- so there the outputs must EQUAL zero.
A zero denominator is torch's 0 / 0 (NaN loss, NaN gradient on the counted rows, 0 on the ignored ones).

Shapes: R at the one-workgroup limit (256) and around it, and three workgroups (the fold); C on both sides of the
K-template switches (64 | 65, 256 | 257) and the group widths 1, 2, 32, 64."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import check_f64, f64_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANGE = 1
NONE, GIVEN, BATCH = 0, 1, 2
IGN = -100
R_EDGES = [1, 255, 256, 257, 515]
C_EDGES = [1, 2, 21, 64, 65, 257]


def _launch(pred, target, mode, weight_in, ignore_index, use_weight=True):
    from graph_hscn import loss as L
    R, C = pred.shape
    counts = torch.full((C,), -7, dtype=torch.int32, device=DEV)
    weight = torch.full((C,), float("nan"), device=DEV)
    denom = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    logp = torch.full_like(pred, float("nan"))
    grad = torch.full_like(pred, float("nan"))
    L.launch_class_weights(target, C, ignore_index, mode, weight_in, counts, weight, denom, flags)
    L.launch_softmax_nll_ex(pred, target, weight if use_weight else None, ignore_index, denom, loss, logp, grad, flags,
                            L.softmax_nll_workspace(R, C, DEV))
    return dict(counts=counts.cpu(), weight=weight.cpu(), denom=float(denom.cpu()), loss=loss.cpu(), logp=logp.cpu(),
                grad=grad.cpu(), flags=int(flags.cpu()))


def _reference(pred, target, weight32, ignore_index):
    """float64 on the CPU; ``target`` holds ``ignore_index`` wherever a row does not count."""
    x = pred.double().requires_grad_(True)
    w = weight32.double()
    loss = F.cross_entropy(x, target, weight=w, ignore_index=ignore_index)
    (grad,) = torch.autograd.grad(loss, x)
    logp = F.log_softmax(x.detach(), dim=-1)
    return loss.detach(), logp, grad


def _logp_mag(pred):
    x64 = pred.double()
    m = x64.max(1, keepdim=True).values
    ls = (x64 - m).exp().sum(1, keepdim=True).log()
    return x64.abs() + m.abs() + ls.abs() + 1.0


def _check(pred, target, mode, weight_in, ignore_index, tag):
    R, C = pred.shape
    got = _launch(pred.to(DEV), target.to(DEV), mode, None if weight_in is None else weight_in.to(DEV), ignore_index,
                  use_weight=mode != NONE)
    counted = (target != ignore_index) & (target >= 0) & (target < C)
    out_of_range = (target != ignore_index) & ~counted
    assert got["flags"] == (RANGE if bool(out_of_range.any()) else 0), tag
    # counts and weights: exact
    n = torch.bincount(target[counted], minlength=C)
    assert torch.equal(got["counts"].long(), n), tag
    V = int(counted.sum())
    if mode == NONE:
        w32 = torch.ones(C)
    elif mode == GIVEN:
        w32 = weight_in.clone()
    else:
        w32 = (V - n).float() / V * (n > 0).float() if V else torch.zeros(C)
    assert torch.equal(got["weight"], w32), tag
    denom64 = 0.0
    for c in range(C):                                   # in class order, as the kernel adds
        denom64 += float(n[c]) * float(w32[c])
    assert got["denom"] == denom64, tag

    clean = torch.where(counted, target, torch.full_like(target, ignore_index))
    x64 = pred.double()
    m = x64.max(1, keepdim=True).values
    logp64 = F.log_softmax(x64, dim=-1)
    logp_mag = _logp_mag(pred)
    if C == 1:
        assert float(got["logp"].abs().max()) == 0.0, tag
    else:
        # row 0 without its largest term in the log-sum-exp
        dropped = logp64.clone()
        rest = (x64[0] - m[0]).exp()
        rest[int(x64[0].argmax())] = 0.0
        dropped[0] = x64[0] - m[0] - rest.sum().log()
        check_f64(got["logp"], logp64, logp_mag, 2 * C + 8, dropped, what=f"{tag} logp")
    if denom64 == 0.0:
        # torch's 0 / 0: NaN loss, NaN on the counted rows, zeros elsewhere
        ref_loss, _, ref_grad = _reference(pred, clean, w32, ignore_index)
        assert bool(torch.isnan(ref_loss)) and bool(torch.isnan(got["loss"]).all()), tag
        assert torch.equal(torch.isnan(got["grad"]), torch.isnan(ref_grad)), tag
        assert float(torch.nan_to_num(got["grad"], nan=0.0).abs().max()) == 0.0, tag
        return got
    loss64, _, grad64 = _reference(pred, clean, w32, ignore_index)
    wy = torch.where(counted, w32.double()[target.clamp(0, C - 1)], torch.zeros(R, dtype=torch.float64))
    onehot = torch.zeros(R, C, dtype=torch.float64)
    onehot[counted, target[counted]] = 1.0
    if C == 1:
        assert float(got["loss"].abs().max()) == 0.0 and float(got["grad"].abs().max()) == 0.0, tag
        return got
    # loss: the row with the largest w |logp| removed
    terms = wy * -(logp64 * onehot).sum(1)
    k = int(terms.abs().argmax())
    loss_mag = float((wy * (logp_mag * onehot).sum(1)).sum()) / denom64
    check_f64(got["loss"].view(()), loss64, loss_mag, R + 2 * C + 12, (terms.sum() - terms[k]) / denom64,
              what=f"{tag} loss")
    # gradient: row k without its onehot
    grad_mag = wy[:, None] * (logp64.exp() + onehot) / denom64
    dropped = grad64.clone()
    dropped[k, int(target[k])] += wy[k] / denom64
    check_f64(got["grad"], grad64, grad_mag, 2 * C + 12, dropped, what=f"{tag} grad")
    assert float(got["grad"][~counted].abs().max()) == 0.0 if bool((~counted).any()) else True, tag
    return got


def _inputs(R, C, seed, absent=False):
    g = torch.Generator().manual_seed(seed)
    hi = C - 1 if absent and C > 2 else C
    return 3.0 * torch.randn(R, C, generator=g), torch.randint(0, hi, (R,), generator=g), g


@pytest.mark.parametrize("C", C_EDGES)
@pytest.mark.parametrize("R", R_EDGES)
def test_weights_and_ignored_rows_against_float64(R, C):
    pred, target, g = _inputs(R, C, 100 * R + C, absent=True)
    given = 0.25 + 2.0 * torch.rand(C, generator=g)
    some = target.clone()
    some[torch.rand(R, generator=g) < 0.3] = IGN
    some[R // 2] = IGN
    for mode, w_in in ((NONE, None), (GIVEN, given), (BATCH, None)):
        for name, t in (("none ignored", target), ("some ignored", some), ("all ignored", torch.full_like(target, IGN))):
            got = _check(pred, t, mode, w_in, IGN, f"R={R} C={C} mode={mode} {name}")
            if mode == BATCH and C > 2 and name == "none ignored":
                assert float(got["weight"][C - 1]) == 0.0 and int(got["counts"][C - 1]) == 0      # the absent class


@pytest.mark.parametrize("R,C", [(9, 5), (257, 21), (515, 65)])
def test_one_target_out_of_range_sets_the_flag_and_adds_nothing(R, C):
    pred, target, g = _inputs(R, C, 7 * R + C)
    target[R - 2] = C
    target[0] = IGN
    given = 0.25 + 2.0 * torch.rand(C, generator=g)
    for mode, w_in in ((NONE, None), (GIVEN, given), (BATCH, None)):
        got = _check(pred, target, mode, w_in, IGN, f"out of range R={R} C={C} mode={mode}")
        assert got["flags"] == RANGE and float(got["grad"][R - 2].abs().max()) == 0.0


def test_an_ignore_index_inside_the_class_range_is_ignored():
    pred, target, _ = _inputs(300, 10, 3)
    got = _check(pred, target, BATCH, None, 1, "ignore_index=1")
    assert int(got["counts"][1]) == 0 and got["flags"] == 0


@pytest.mark.parametrize("R,C", [(r, c) for r in R_EDGES for c in C_EDGES])
def test_without_weights_and_ignored_rows_the_bits_are_the_unweighted_kernel_s(R, C):
    from graph_hscn import loss as L
    pred, target, _ = _inputs(R, C, 31 * R + C)
    pred, target = pred.to(DEV), target.to(DEV)
    loss, logp, grad = torch.empty(1, device=DEV), torch.empty_like(pred), torch.empty_like(pred)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.launch_softmax_nll(pred, target, loss, logp, grad, flags, L.softmax_nll_workspace(R, C, DEV))
    got = _launch(pred, target, NONE, None, IGN, use_weight=False)
    assert got["denom"] == float(R)
    assert torch.equal(got["loss"], loss.cpu()) and torch.equal(got["logp"], logp.cpu())
    assert torch.equal(got["grad"], grad.cpu())


@pytest.mark.parametrize("R,C", [(257, 21), (515, 65)])
def test_two_calls_give_the_same_bits(R, C):
    pred, target, g = _inputs(R, C, 5)
    target[torch.rand(R, generator=g) < 0.2] = IGN
    pred, target = pred.to(DEV), target.to(DEV)
    a, b = _launch(pred, target, BATCH, None, IGN), _launch(pred, target, BATCH, None, IGN)
    for k in ("counts", "weight", "loss", "logp", "grad"):
        assert torch.equal(a[k], b[k]), k
    assert a["denom"] == b["denom"]


@pytest.mark.parametrize("R,C", [(128, 10), (600, 21)])
def test_criterion_with_class_weights_on_the_device(R, C):
    from graph_hscn.loss import LazyScaled, check_class_targets, criterion
    pred_cpu, target, g = _inputs(R, C, 41, absent=True)
    target[torch.rand(R, generator=g) < 0.25] = IGN
    given = 0.25 + 2.0 * torch.rand(C, generator=g)
    for kw in (dict(class_weight="batch"), dict(class_weight=given), dict(ignore_index=IGN)):
        kw.setdefault("ignore_index", IGN)
        ref_loss, ref_score = criterion("cross_entropy", pred_cpu.double(), target, **kw)      # the CPU restatement
        x = pred_cpu.double().requires_grad_(True)
        (ref_grad,) = torch.autograd.grad(criterion("cross_entropy", x, target, **kw)[0], x)
        pred = pred_cpu.to(DEV).requires_grad_(True)
        loss, score = criterion("cross_entropy", pred, target.to(DEV), **kw)
        assert loss.dim() == 0 and loss.requires_grad and not score.requires_grad
        # the bounds of the module docstring, from the reference's own weights: ref_grad's onehot entry is
        # -w_y (1 - p) / denom, so w_y / denom = -(sum over the row of the negative entries) / (1 - p_y)
        counted = target != IGN
        logp_mag = _logp_mag(pred_cpu)
        p64 = ref_score.exp()
        onehot = torch.zeros(R, C, dtype=torch.float64)
        onehot[counted, target[counted]] = 1.0
        wy_over_denom = (-(ref_grad * onehot).sum(1) / (1.0 - (p64 * onehot).sum(1))).clamp_min(0.0)
        loss_mag = float((wy_over_denom * (logp_mag * onehot).sum(1)).sum())
        assert f64_close(loss, ref_loss, loss_mag, R + 2 * C + 12, what="criterion loss")
        assert f64_close(score, ref_score, logp_mag, 2 * C + 8, what="criterion score")
        (2.5 * loss).backward()
        assert not isinstance(pred.grad, LazyScaled)
        grad_mag = 2.5 * wy_over_denom[:, None] * (p64 + onehot)
        assert f64_close(pred.grad, 2.5 * ref_grad, grad_mag, 2 * C + 13, what="criterion grad")
    lw, _ = criterion("weighted_cross_entropy", pred_cpu.to(DEV), target.clamp_min(0).to(DEV))
    lb, _ = criterion("cross_entropy", pred_cpu.to(DEV), target.clamp_min(0).to(DEV), class_weight="batch")
    assert torch.equal(lw, lb)
    check_class_targets(DEV)
