"""Loss selection of the training loop (reference graph_hscn/loss.py:6-19).

On the device the multilabel BCE-with-logits and L1 branches are one fused HIP
launch (loss + sigmoid score + dL/dpred, csrc/loss.hip) -- or none at all: a prediction
of the graph-resident HSCN forward arrives with its score, and the loss and its gradient
are evaluated inside the backward launch of the same step (``LazyLoss``).  The multiclass branch
(``true.ndim == 1``: class-index targets) is one fused launch as well (log-softmax + NLL: loss, the
log-probabilities it returns as the score, dL/dpred; ``hscn_softmax_nll_fwd``).  CPU tensors use the
plain torch ops the reference uses.  Class weights and ``ignore_index`` (``criterion(..., class_weight=,
ignore_index=)``, ``loss_fn="weighted_cross_entropy"``: LRGB's per-batch weights) are two calls on the device --
``hscn_class_weights`` leaves the counts, the weights and the denominator there, ``hscn_softmax_nll_fwd_ex`` divides by
it -- and ``F.cross_entropy`` with the same weights on the CPU.  Quirk kept: the L1 branch scores with ``sigmoid(pred)``
(loss.py:17-19).

A class index outside ``[0, C)`` raises ``IndexError`` in torch at once; the launch cannot raise, it
sets a bit in a per-device flag word (``class_target_flags``) and leaves the row out of the loss.  The
word is read -- one synchronising copy -- by ``check_class_targets(device)``, which raises the
``IndexError`` and clears it: ``train.train_resident.fit_resident`` calls it at the end of every epoch's
read-back, ``train.eval_resident.DeviceEvaluator.evaluate`` brings the word over with its loss and
metric.  ``step.ResidentTrainStep`` keeps a word of its own, read by its ``check()``."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from ._hip import FlagWord, call, lib, ptr, stream


class LazyScaled(torch.Tensor):
    """``scale[0] * grad`` not yet multiplied out.  The loss node returns its input gradient in this
    form; a consumer that can apply the scalar itself (the graph-resident HSCN backward takes it as
    ``g_scale``) reads ``.grad_unscaled`` / ``.scale`` and no scaling launch happens; any other use
    (an ordinary torch op, a hook, gradient accumulation) dispatches through ``materialize``."""

    @staticmethod
    def __new__(cls, grad, scale):
        r = torch.Tensor._make_wrapper_subclass(cls, grad.shape, dtype=grad.dtype, device=grad.device,
                                                requires_grad=False)
        r.grad_unscaled = grad
        r.scale = scale
        r._dense = None
        return r

    def materialize(self) -> torch.Tensor:
        if self._dense is None:
            out = torch.empty_like(self.grad_unscaled)
            call("hscn_scale", ptr(self.scale), ptr(self.grad_unscaled), ptr(out), out.numel(), stream())
            self._dense = out
        return self._dense

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        un = lambda t: t.materialize() if isinstance(t, LazyScaled) else t
        return func(*tree_map(un, args), **tree_map(un, kwargs or {}))

    def __repr__(self):
        return f"LazyScaled(shape={tuple(self.shape)})"


def _run_criterion(pred, true, kind, want_score=True):
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    score = torch.empty_like(pred) if want_score else None
    grad = torch.empty_like(pred)
    call("hscn_criterion_fwd", ptr(pred), ptr(true), pred.numel(), kind, ptr(loss), ptr(score), ptr(grad), stream())
    return loss.view(()), score, grad


class _LossState:
    """A loss whose evaluation was left to the backward launch of the graph-resident HSCN step
    (include/hscn.h: hscn_loss_tail).  ``value`` appears when that launch has been issued (``fill``); a
    read before that -- ``loss.item()`` ahead of ``backward()``, or no backward at all -- evaluates the
    loss with a launch of its own and keeps its gradient for the backward."""
    __slots__ = ("pred", "target", "kind", "value", "grad")

    def __init__(self, pred, target, kind):
        # VALUES only: the state outlives the step (``loss.detach()`` of a LazyLoss shares it, and a training loop
        # collects those, train/train.py:85), so it must not hold the prediction's autograd graph -- that kept every
        # iteration's saved activations alive until the epoch ended, and the parameters' gradient-accumulation
        # nodes with them (round 1: the precursor of the capture_end crash)
        self.pred, self.target, self.kind = pred.detach(), target.detach(), kind
        self.value = self.grad = None

    def fill(self, value):
        self.value = value

    def get(self):
        if self.value is None:
            self.value, _, self.grad = _run_criterion(self.pred, self.target, self.kind, want_score=False)
        return self.value


_ONES = {}


def root_grad(device):
    """Cached scalar 1 on ``device``: ``loss.backward(root_grad(dev))`` spares the fill launch of the
    implicit ``ones_like(loss)`` (4.5 us per step on a 50 us step)."""
    return _one(torch.device(device))


def _one(device):
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones((), dtype=torch.float32, device=device)
    return t


class LazyLoss(torch.Tensor):
    """0-dim loss backed by a ``_LossState``: any use as a value dispatches through ``state.get()``;
    ``detach`` / ``alias`` stay lazy (a training loop may collect ``loss.detach()`` before ``backward()``),
    and ``ones_like`` -- the implicit root gradient of ``loss.backward()`` -- does not need the value."""

    @staticmethod
    def __new__(cls, state, device):
        r = torch.Tensor._make_wrapper_subclass(cls, (), dtype=torch.float32, device=device, requires_grad=False)
        r.state = state
        return r

    def materialize(self) -> torch.Tensor:
        return self.state.get()

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        if func in (torch.ops.aten.detach.default, torch.ops.aten.alias.default):
            return LazyLoss(args[0].state, args[0].device)
        if func is torch.ops.aten.ones_like.default and (kwargs or {}).get("dtype") in (None, torch.float32):
            return _one(args[0].device)        # (the implicit root gradient of loss.backward())
        un = lambda t: t.state.get() if isinstance(t, LazyLoss) else t
        return func(*tree_map(un, args), **tree_map(un, kwargs or {}))

    def __repr__(self):
        return f"LazyLoss({'pending' if self.state.value is None else float(self.state.value)})"


class LazyCriterionGrad(torch.Tensor):
    """``scale[0] * d criterion(pred, target) / d pred`` not yet evaluated: the graph-resident HSCN backward
    takes (pred, target, kind, scale) and evaluates it inside its launch; anything else gets the dense
    tensor through ``materialize``."""

    @staticmethod
    def __new__(cls, pred, target, kind, scale, state):
        r = torch.Tensor._make_wrapper_subclass(cls, pred.shape, dtype=pred.dtype, device=pred.device,
                                                requires_grad=False)
        r.pred, r.target, r.kind, r.scale, r.state = pred, target, kind, scale, state
        r._dense = None
        return r

    def materialize(self) -> torch.Tensor:
        if self._dense is None:
            self.state.get()
            out = torch.empty_like(self.state.grad)
            call("hscn_scale", ptr(self.scale), ptr(self.state.grad), ptr(out), out.numel(), stream())
            self._dense = out
        return self._dense

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        un = lambda t: t.materialize() if isinstance(t, LazyCriterionGrad) else t
        return func(*tree_map(un, args), **tree_map(un, kwargs or {}))

    def __repr__(self):
        return f"LazyCriterionGrad(shape={tuple(self.shape)})"


class _TailCriterionFn(Function):
    """criterion on a prediction of the graph-resident HSCN forward (which already wrote the score):
    no launch here; the backward launch of the step evaluates the loss tail (csrc/resident.hip)."""

    @staticmethod
    def forward(ctx, pred, true, kind):
        ctx.state = _LossState(pred, true, kind)
        ctx.set_materialize_grads(False)
        return LazyLoss(ctx.state, pred.device)

    @staticmethod
    def backward(ctx, g_loss):
        if g_loss is None:
            return None, None, None
        st = ctx.state
        scale = g_loss.reshape(1).contiguous()
        if st.grad is not None:                  # the loss was read before the backward: its gradient exists
            return LazyScaled(st.grad, scale), None, None
        return LazyCriterionGrad(st.pred, st.target, st.kind, scale, st), None, None


class _CriterionFn(Function):
    @staticmethod
    def forward(ctx, pred, true, kind):
        loss, score, grad = _run_criterion(pred.contiguous(), true.contiguous(), kind)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(score)
        ctx.set_materialize_grads(False)  # no zero tensor (a fill launch) for the score output
        return loss, score

    @staticmethod
    def backward(ctx, g_loss, _g_score):
        (grad,) = ctx.saved_tensors
        if g_loss is None:
            return None, None, None
        return LazyScaled(grad, g_loss.reshape(1).contiguous()), None, None


# bits of hscn_softmax_nll_fwd's ``flags`` (include/hscn.h).  Only the first becomes an error here: a NaN prediction
# makes the loss itself NaN, as in torch, so NAN_PRED is there for a caller that reads the word, nothing raises on it
TARGET_OUT_OF_RANGE, NAN_PRED = 1, 2
_NLL_FLAGS = FlagWord()


def class_target_flags(device) -> torch.Tensor:
    """The device's flag word [1] int32 that every multiclass ``criterion`` call ORs its bits into."""
    return _NLL_FLAGS.of(device)


def raise_for_class_flags(flags: int) -> None:
    if flags & TARGET_OUT_OF_RANGE:
        raise IndexError("Target out of bounds: a class index outside [0, C) reached the multiclass criterion")


def check_class_targets(device) -> None:
    """Synchronising: read and clear the device's flag word; ``IndexError`` if a multiclass ``criterion`` call since
    the last check met a class index outside ``[0, C)`` (torch's own error for it, raised late).  A ``NAN_PRED`` bit
    is cleared with it and raises nothing: the loss of that call is NaN already."""
    raise_for_class_flags(_NLL_FLAGS.take(device))


def softmax_nll_workspace(R: int, C: int, device):
    """The launch's scratch (None where it needs none: ``R`` up to one workgroup's rows)."""
    nbytes = int(lib().hscn_softmax_nll_workspace_bytes(R, C))
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def launch_softmax_nll(pred, true, loss, logp, grad, flags, workspace) -> None:
    """``hscn_softmax_nll_fwd`` on ``pred`` [R, C] float32 / ``true`` [R] int64 into preallocated outputs."""
    R, C = pred.shape
    call("hscn_softmax_nll_fwd", ptr(pred), ptr(true), R, C, ptr(loss), ptr(logp), ptr(grad), ptr(flags),
         ptr(workspace), workspace.numel() if workspace is not None else 0, stream())


class _SoftmaxNllFn(Function):
    """The multiclass branch: one launch for loss, log-probabilities and dL/dpred; the backward is a scale the
    consumer may apply itself (``LazyScaled``), exactly as ``_CriterionFn``'s."""

    @staticmethod
    def forward(ctx, pred, true):
        pred, true = pred.contiguous(), true.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        # (the launch always writes dL/dpred -- include/hscn.h: only logp is optional -- so the buffer exists under
        # no_grad too, where nothing reads it; it goes back to the caching allocator when forward returns)
        logp, grad = torch.empty_like(pred), torch.empty_like(pred)
        launch_softmax_nll(pred, true, loss, logp, grad, class_target_flags(pred.device),
                           softmax_nll_workspace(pred.size(0), pred.size(1), pred.device))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(logp)
        ctx.set_materialize_grads(False)
        return loss.view(()), logp

    @staticmethod
    def backward(ctx, g_loss, _g_logp):
        (grad,) = ctx.saved_tensors
        if g_loss is None:
            return None, None
        return LazyScaled(grad, g_loss.reshape(1).contiguous()), None


def _multiclass_on_device(pred: torch.Tensor, true: torch.Tensor) -> bool:
    return (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2 and true.dtype == torch.int64
            and true.device == pred.device and true.size(0) == pred.size(0) and pred.numel() > 0)


CW_NONE, CW_GIVEN, CW_BATCH = 0, 1, 2       # `mode` of hscn_class_weights (include/hscn.h)
_NO_IGNORE = -(1 << 63)                      # an ignore_index no int64 target written by a loader takes: nothing ignored


def launch_class_weights(true, C, ignore_index, mode, weight_in, counts, weight, denom, flags) -> None:
    """``hscn_class_weights`` on ``true`` [R] int64 into preallocated ``counts`` [C] int32, ``weight`` [C] float32 and
    ``denom`` [1] float64."""
    call("hscn_class_weights", ptr(true), true.numel(), C, ignore_index, mode, ptr(weight_in), ptr(counts), ptr(weight),
         ptr(denom), ptr(flags), stream())


def launch_softmax_nll_ex(pred, true, weight, ignore_index, denom, loss, logp, grad, flags, workspace) -> None:
    """``hscn_softmax_nll_fwd_ex`` into preallocated outputs; ``denom`` is what ``launch_class_weights`` wrote."""
    R, C = pred.shape
    call("hscn_softmax_nll_fwd_ex", ptr(pred), ptr(true), R, C, ptr(weight), ignore_index, ptr(denom), ptr(loss),
         ptr(logp), ptr(grad), ptr(flags), ptr(workspace), workspace.numel() if workspace is not None else 0, stream())


def _weight_mode(class_weight, C, device):
    """``(mode, weight_in)`` of ``hscn_class_weights`` for a ``class_weight`` of None, "batch" or a [C] tensor."""
    if class_weight is None:
        return CW_NONE, None
    if isinstance(class_weight, str):
        if class_weight != "batch":
            raise ValueError(f"class_weight must be None, 'batch' or a [C] tensor, not {class_weight!r}")
        return CW_BATCH, None
    w = torch.as_tensor(class_weight)
    if w.dim() != 1 or w.numel() != C:
        raise ValueError(f"class_weight must have one entry per class ({C}), got shape {tuple(w.shape)}")
    return CW_GIVEN, w.to(device=device, dtype=torch.float32).contiguous()


class _WeightedSoftmaxNllFn(Function):
    """The multiclass branch with class weights and / or ``ignore_index``: the counts, the weights and the
    denominator stay on the device (``hscn_class_weights``), the fused row launch divides by it
    (``hscn_softmax_nll_fwd_ex``); the backward is ``_SoftmaxNllFn``'s."""

    @staticmethod
    def forward(ctx, pred, true, mode, weight_in, ignore_index):
        pred, true = pred.contiguous(), true.contiguous()
        dev, (R, C) = pred.device, pred.shape
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        logp, grad = torch.empty_like(pred), torch.empty_like(pred)
        counts = torch.empty(C, dtype=torch.int32, device=dev)
        weight = torch.empty(C, dtype=torch.float32, device=dev)
        denom = torch.empty(1, dtype=torch.float64, device=dev)
        flags = class_target_flags(dev)
        launch_class_weights(true, C, ignore_index, mode, weight_in, counts, weight, denom, flags)
        launch_softmax_nll_ex(pred, true, None if mode == CW_NONE else weight, ignore_index, denom, loss, logp, grad,
                              flags, softmax_nll_workspace(R, C, dev))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(logp)
        ctx.set_materialize_grads(False)
        return loss.view(()), logp

    @staticmethod
    def backward(ctx, g_loss, _g_logp):
        (grad,) = ctx.saved_tensors
        if g_loss is None:
            return None, None, None, None, None
        return LazyScaled(grad, g_loss.reshape(1).contiguous()), None, None, None, None


def batch_class_weights(true: torch.Tensor, C: int, ignore_index=None) -> torch.Tensor:
    """LRGB's ``weighted_cross_entropy`` weights in plain torch ops: with V the counted rows and n_c the rows of class
    c, ``(V - n_c).float() / V`` on the classes present and 0 elsewhere."""
    kept = true if ignore_index is None else true[true != ignore_index]
    n = torch.bincount(kept, minlength=C)[:C]
    V = int(kept.numel())
    return (V - n).float() / V * (n > 0).float()


def _weighted_cross_entropy_torch(pred, true, class_weight, ignore_index):
    """The rule of the device path restated with torch ops (CPU tensors; the reference of the tests)."""
    C = pred.size(-1)
    if isinstance(class_weight, str):
        if class_weight != "batch":
            raise ValueError(f"class_weight must be None, 'batch' or a [C] tensor, not {class_weight!r}")
        weight = batch_class_weights(true, C, ignore_index).to(pred.dtype)
    else:
        weight = None if class_weight is None else torch.as_tensor(class_weight).to(device=pred.device, dtype=pred.dtype)
    logp = F.log_softmax(pred, dim=-1)
    loss = F.cross_entropy(pred, true, weight=weight, ignore_index=-100 if ignore_index is None else ignore_index)
    return loss, logp


def criterion(loss_fn: str, pred: torch.Tensor, true: torch.Tensor, *, class_weight=None, ignore_index=None):
    """``class_weight`` / ``ignore_index`` (extensions, class-index targets only): ``F.cross_entropy``'s ``weight``
    and ``ignore_index``; ``class_weight="batch"`` derives the weights from the batch's own class counts (LRGB's
    ``weighted_cross_entropy``), which ``loss_fn="weighted_cross_entropy"`` selects by itself."""
    if loss_fn == "weighted_cross_entropy":
        if true.ndim != 1 or pred.ndim != 2:
            raise ValueError("weighted_cross_entropy takes class-index targets [R] and a prediction [R, C]")
        loss_fn = "cross_entropy"
        if class_weight is None:
            class_weight = "batch"
    multiclass = loss_fn == "cross_entropy" and pred.ndim > 1 and true.ndim == 1
    if class_weight is not None or ignore_index is not None:
        if not multiclass:
            raise ValueError("class_weight / ignore_index belong to the multiclass criterion (cross_entropy on "
                             "class-index targets)")
        if _multiclass_on_device(pred, true):
            mode, weight_in = _weight_mode(class_weight, pred.size(1), pred.device)
            return _WeightedSoftmaxNllFn.apply(pred, true, mode, weight_in,
                                               _NO_IGNORE if ignore_index is None else int(ignore_index))
        if pred.is_cuda:
            raise RuntimeError("the weighted multiclass criterion on the device takes a float32 [R, C] prediction and "
                               "int64 [R] targets on the same device")
        return _weighted_cross_entropy_torch(pred, true, class_weight, ignore_index)
    if multiclass and _multiclass_on_device(pred, true):
        return _SoftmaxNllFn.apply(pred, true)
    if pred.is_cuda and not multiclass and pred.dtype == torch.float32 and pred.shape == true.shape:
        kind = 0 if loss_fn == "cross_entropy" else 1
        true = true.float()
        score = getattr(pred, "_hscn_score", None)
        if score is not None:                                   # (score, version of pred it belongs to)
            score = score[0] if score[1] == pred._version else None
        if (score is not None and pred.requires_grad and torch.is_grad_enabled() and pred.dim() == 2
                and true.is_contiguous() and pred.is_contiguous() and true.device == pred.device):
            _one(pred.device)          # the root gradient of loss.backward(), created outside any capture
            return _TailCriterionFn.apply(pred, true, kind), score
        return _CriterionFn.apply(pred, true, kind)
    if loss_fn == "cross_entropy":
        if multiclass:
            pred = F.log_softmax(pred, dim=-1)
            return F.nll_loss(pred, true), pred
        true = true.float()
        return F.binary_cross_entropy_with_logits(pred, true, reduction="mean"), torch.sigmoid(pred)
    return F.l1_loss(pred, true), torch.sigmoid(pred)
