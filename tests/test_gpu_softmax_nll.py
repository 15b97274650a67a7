"""hscn_softmax_nll_fwd (csrc/loss.hip) and the criterion's multiclass branch on the device against torch on the CPU
in float64 (``F.log_softmax`` / ``F.nll_loss`` and their autograd).

Bounds (the issue's; tests/test_gpu_ops_f64.py constructs no per-op bound for a softmax, so none tighter is taken
from there): |logp - logp64| <= 1e-5 (the project's activation tolerance) -- scaled by max(1, |pred|max / 10) in the
+-80 case only --, |grad - grad64| * R <= 1e-5, |loss - loss64| <= 1e-5 * max(1, |loss64|).

The kernel's edges (csrc/loss.hip): lane-group widths 1, 2, 4, ..., 64 (C = each width and one past it), 1 / 4 / 16
columns per lane (C <= 64 / 256 / 1024 = the cap), 256 rows per workgroup (R = 256 is one launch, 257 takes the
partial-sum fold), 1024 / width rows in flight per pass."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
RANGE, NAN = 1, 2
MAX_C = 1024
SLAB = 256


def _launch(pred, target, want_logp=True):
    from graph_hscn._hip import call, lib, ptr, stream
    R, C = pred.shape
    loss = torch.full((1,), float("nan"), device=DEV)
    logp = torch.full_like(pred, float("nan")) if want_logp else None
    grad = torch.full_like(pred, float("nan"))
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = int(lib().hscn_softmax_nll_workspace_bytes(R, C))
    assert nbytes == (0 if R <= SLAB else 4 * ((R + SLAB - 1) // SLAB))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    call("hscn_softmax_nll_fwd", ptr(pred), ptr(target), R, C, ptr(loss), ptr(logp), ptr(grad), ptr(flags), ptr(ws),
         nbytes, stream())
    return loss, logp, grad, flags


def _reference(pred_cpu, target_cpu):
    x = pred_cpu.double().requires_grad_(True)
    logp = F.log_softmax(x, dim=-1)
    loss = F.nll_loss(logp, target_cpu)
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), logp.detach(), grad


def _check(pred_cpu, target_cpu, got, scale=1.0, tag=""):
    loss, logp, grad, flags = got
    R = pred_cpu.size(0)
    loss64, logp64, grad64 = _reference(pred_cpu, target_cpu)
    d_logp = float((logp.cpu().double() - logp64).abs().max())
    d_grad = float((grad.cpu().double() - grad64).abs().max()) * R
    d_loss = abs(float(loss.cpu().double()) - float(loss64))
    print(f"[softmax-nll {tag} R={R} C={pred_cpu.size(1)}] |dlogp| {d_logp:.3e} (bound {1e-5 * scale:.1e})  "
          f"|dgrad| R {d_grad:.3e}  |dloss| {d_loss:.3e} (loss {float(loss64):.4f})")
    assert int(flags.item()) == 0
    assert d_logp <= 1e-5 * scale
    assert d_grad <= 1e-5
    assert d_loss <= 1e-5 * max(1.0, abs(float(loss64)))


def _inputs(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(R, C, generator=g), torch.randint(0, C, (R,), generator=g)


# widths 1..64 at and past each, the per-lane column counts at and past each, the cap
C_EDGES = [1, 2, 3, 4, 5, 8, 9, 10, 16, 17, 32, 33, 63, 64, 65, 256, 257, MAX_C - 1, MAX_C]
# one row; around a wave of rows; one workgroup's slab below / at / past; a few workgroups (the last one partial)
R_EDGES = [1, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 41]


@pytest.mark.parametrize("C", C_EDGES)
def test_against_float64_over_the_class_widths(C):
    for R in (1, 65, SLAB + 1):
        pred, target = _inputs(R, C, 1000 * C + R)
        _check(pred, target, _launch(pred.to(DEV), target.to(DEV)), tag="widths")


@pytest.mark.parametrize("R", R_EDGES)
def test_against_float64_over_the_row_counts(R):
    for C in (1, 2, 10, 16, 17, 64):
        pred, target = _inputs(R, C, 7 * R + C)
        _check(pred, target, _launch(pred.to(DEV), target.to(DEV)), tag="rows")


def test_rows_of_equal_logits_and_logits_a_naive_exp_overflows():
    pred, target = _inputs(70, 10, 5)
    pred[3] = 1.25                                       # a row of equal logits: logp = -log C
    pred[69] = 0.0
    got = _launch(pred.to(DEV), target.to(DEV))
    _check(pred, target, got, tag="equal row")
    assert float((got[1][3].cpu().double() + torch.log(torch.tensor(10.0, dtype=torch.float64))).abs().max()) <= 1e-6
    for C in (10, 65):
        g = torch.Generator().manual_seed(C)
        pred = torch.where(torch.rand(300, C, generator=g) < 0.5, -80.0, 80.0)
        pred[0] = 80.0
        pred[1] = -80.0
        pred[2, 1:] = -80.0
        target = torch.randint(0, C, (300,), generator=g)
        got = _launch(pred.to(DEV), target.to(DEV))
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        _check(pred, target, got, scale=max(1.0, float(pred.abs().max()) / 10.0), tag="+-80")


@pytest.mark.parametrize("R,C", [(128, 10), (SLAB + 1, 17), (3 * SLAB + 41, 65)])
def test_two_launches_give_the_same_bits(R, C):
    pred, target = _inputs(R, C, 11)
    pred, target = pred.to(DEV), target.to(DEV)
    a, b = _launch(pred, target), _launch(pred, target)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    c = _launch(pred, target, want_logp=False)           # logp is optional
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2])


@pytest.mark.parametrize("R,C", [(9, 5), (SLAB + 7, 10)])
def test_targets_out_of_range_set_the_flag_and_leave_the_other_rows_right(R, C):
    pred, target = _inputs(R, C, 21)
    bad = target.clone()
    bad[2], bad[R - 1] = -1, C
    loss, logp, grad, flags = _launch(pred.to(DEV), bad.to(DEV))
    torch.cuda.synchronize()
    assert int(flags.item()) == RANGE
    keep = torch.ones(R, dtype=torch.bool)
    keep[2] = keep[R - 1] = False
    _, logp64, _ = _reference(pred, target)
    assert float((logp.cpu().double() - logp64).abs().max()) <= 1e-5       # every row's logp, the bad rows' too
    # the other rows: the loss and gradient of the mean over R with the bad rows contributing nothing
    x = pred.double().requires_grad_(True)
    lp = F.log_softmax(x, dim=-1)
    loss64 = -(lp[keep].gather(1, target[keep, None]).sum()) / R
    (grad64,) = torch.autograd.grad(loss64, x)
    assert abs(float(loss.cpu()) - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64)))
    assert float((grad.cpu().double() - grad64).abs().max()) * R <= 1e-5
    assert float(grad.cpu()[~keep].abs().max()) == 0.0


def test_nan_sets_the_nan_bit():
    pred, target = _inputs(40, 10, 31)
    pred[17, 4] = float("nan")
    loss, logp, grad, flags = _launch(pred.to(DEV), target.to(DEV))
    assert int(flags.item()) == NAN
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(logp[17]).all())
    assert bool(torch.isfinite(logp[:17]).all()) and bool(torch.isfinite(logp[18:]).all())


def test_bad_arguments_are_refused_before_any_launch():
    from graph_hscn import _hip
    L = _hip.lib()
    p = _hip.ptr(torch.zeros(64, device=DEV))
    nll = L.hscn_softmax_nll_fwd
    assert nll(p, p, 0, 4, p, None, p, p, None, 0, None) == -1
    assert nll(p, p, 4, 4, None, None, p, p, None, 0, None) == -1
    assert nll(p, p, 4, 4, p, None, None, p, None, 0, None) == -1
    assert nll(p, p, 4, MAX_C + 1, p, None, p, p, None, 0, None) == -1
    assert nll(p, p, SLAB + 1, 4, p, None, p, p, None, 0, None) == -1
    assert nll(p, p, SLAB + 1, 4, p, None, p, p, p, 4, None) == -2
    torch.cuda.synchronize()


@pytest.mark.parametrize("R,C", [(1, 3), (128, 10), (SLAB + 44, 16)])
def test_criterion_on_the_device(R, C):
    from graph_hscn.loss import LazyScaled, check_class_targets, criterion
    pred_cpu, target = _inputs(R, C, 41)
    loss64, logp64, grad64 = _reference(pred_cpu, target)
    for root in (None, 2.5):
        pred = pred_cpu.to(DEV).requires_grad_(True)
        loss, score = criterion("cross_entropy", pred, target.to(DEV))
        assert loss.dim() == 0 and not score.requires_grad and loss.requires_grad
        assert abs(float(loss.detach().cpu()) - float(loss64)) <= 1e-5 * max(1.0, abs(float(loss64)))
        assert float((score.cpu().double() - logp64).abs().max()) <= 1e-5
        (loss if root is None else root * loss).backward()
        assert not isinstance(pred.grad, LazyScaled)
        d = float((pred.grad.cpu().double() - (root or 1.0) * grad64).abs().max()) * R
        assert d <= 1e-5, d
    check_class_targets(DEV)                             # nothing flagged
    with torch.no_grad():                                # out of range: IndexError where the flag is read
        criterion("cross_entropy", pred_cpu.to(DEV), torch.full((R,), C, device=DEV))
    with pytest.raises(IndexError):
        check_class_targets(DEV)
    check_class_targets(DEV)                             # (read and cleared)
