"""Epoch metrics of the training loop (reference graph_hscn/metrics.py:6-36), computed where the
tensors live: the reference moves every epoch's `[N, C]` labels and scores to the host and loops
over classes in sklearn; here the sort / cumulative sums run on the device (plain torch ops, they
are not on the hot path) and one scalar comes back.  Same definitions and error behaviour:
``eval_ap`` = mean over the classes that have both a positive and a negative label of sklearn's
``average_precision_score`` (step-wise integral of the precision-recall curve over distinct score
thresholds, NaN labels ignored); ``eval_mae`` = mean absolute error, raising on NaN predictions.

Class-index targets (the criterion's multiclass branch; the reference has no metric for them): ``eval_accuracy`` and
``eval_f1_macro`` on ``y_true`` [G] int64 and ``y_pred`` [G, C] scores (logits or log-probabilities).  The predicted
class is the FIRST maximal column (numpy's ``argmax``); macro-F1 is scikit-learn's ``f1_score(average="macro")``:
the mean over the labels present in ``y_true`` or the predictions, a class without a true positive counting 0."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _hip


def _ap_one(y: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """sklearn.metrics.average_precision_score for one binary column (float64)."""
    order = torch.argsort(s, descending=True, stable=True)
    s, y = s[order], y[order]
    tp = torch.cumsum(y, 0)
    n = torch.arange(1, y.numel() + 1, dtype=torch.float64, device=y.device)
    last = torch.ones_like(s, dtype=torch.bool)          # last element of every run of equal scores
    last[:-1] = s[1:] != s[:-1]
    precision = (tp / n)[last]
    recall = (tp / tp[-1])[last]
    prev = torch.cat([recall.new_zeros(1), recall[:-1]])
    return ((recall - prev) * precision).sum()


def eval_ap(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:      # metrics.py:6-27
    y_true = y_true.detach().to(torch.float64)
    y_pred = y_pred.detach().to(torch.float64)
    aps = []
    for i in range(y_true.shape[1]):
        col = y_true[:, i]
        if bool((col == 1).any()) and bool((col == 0).any()):
            labeled = col == col                                          # ignore NaN labels
            aps.append(_ap_one(col[labeled], y_pred[labeled, i]))
    if not aps:
        raise RuntimeError("No positively labeled data available. Cannot compute Average"
                           "Precision.")
    return float(torch.stack(aps).sum().item() / len(aps))


def eval_mae(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:     # metrics.py:30-36
    y_pred = y_pred.detach()
    if bool(torch.isnan(y_pred).any()):
        raise Exception("Model is predicting NaN.")
    d = (y_true.detach().to(torch.float64) - y_pred.to(torch.float64)).abs()
    return float(d.mean().item())


def _first_argmax(y_pred: torch.Tensor) -> torch.Tensor:
    """Index of the first maximal column of every row (``torch.argmax`` does not promise which of several)."""
    C = y_pred.size(1)
    cols = torch.arange(C, device=y_pred.device).expand_as(y_pred)
    top = y_pred == y_pred.max(dim=1, keepdim=True).values
    return torch.where(top, cols, torch.full_like(cols, C)).min(dim=1).values


def _class_inputs(y_true: torch.Tensor, y_pred: torch.Tensor):
    y_true, y_pred = y_true.detach(), y_pred.detach()
    if y_true.dim() != 1 or y_pred.dim() != 2 or y_true.size(0) != y_pred.size(0) or y_pred.numel() == 0:
        raise ValueError("y_true must be [G] class indices and y_pred non-empty [G, C] scores")
    if y_true.dtype.is_floating_point or y_true.dtype == torch.bool:
        raise TypeError("y_true must hold integer class indices")
    if bool(torch.isnan(y_pred).any()):
        raise ValueError("Input contains NaN.")
    return y_true.to(torch.int64), y_pred


def confusion_matrix(y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    """[C, C] int64, rows = true class, columns = predicted class (first maximal column)."""
    y_true, y_pred = _class_inputs(y_true, y_pred)
    C = y_pred.size(1)
    if bool(((y_true < 0) | (y_true >= C)).any()):
        raise IndexError("Target out of bounds: a class index outside [0, C)")
    flat = torch.bincount(y_true * C + _first_argmax(y_pred), minlength=C * C)
    return flat.view(C, C)


def eval_accuracy(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    conf = confusion_matrix(y_true, y_pred)
    return float(conf.diagonal().sum().item()) / float(y_true.size(0))


def eval_f1_macro(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    conf = confusion_matrix(y_true, y_pred).to(torch.float64)
    tp = conf.diagonal()
    support = conf.sum(1) + conf.sum(0)                  # rows with that target + rows with that prediction
    present = support > 0
    f1 = torch.where(tp > 0, 2.0 * tp / support.clamp(min=1.0), torch.zeros_like(tp))
    total = 0.0
    for v in f1[present].tolist():                       # in class order, as hscn_multiclass_metrics adds them
        total += v
    return total / float(present.sum().item())


# ---- the same two metrics as HIP launches (csrc/metrics.hip; include/hscn.h) ------------------------------------------
# ``eval_ap`` / ``eval_mae`` above read back per class; these sort and scan every class in one launch and the host
# reads ``result`` and ``flags`` once, together.

NO_VALID_CLASS, NAN_INPUT, TARGET_OUT_OF_RANGE = 1, 2, 4       # bits of ``flags`` (include/hscn.h)
CLASS_METRICS = ("accuracy", "f1_macro")       # hscn_multiclass_metrics: result[0] / result[1]
METRICS = ("ap", "mae") + CLASS_METRICS
_PACKED_BYTES = 32                     # result [2] f64 | flags [1] i32 | 3 spare 32-bit words, ONE buffer = one copy


class MetricResult(NamedTuple):
    """Device tensors of a metric launch.  ``result`` [2] float64 = (the metric, the number of valid classes -- for
    the MAE the element count; for the class-index metrics (accuracy, macro-F1), see ``result_index``), ``flags`` [1]
    int32; ``ap`` [C] float64 and ``valid`` [C] int32 per class (``None`` for the MAE; for the class-index metrics the
    per-class F1 and the [C, C] int32 confusion matrix).  ``result`` and ``flags`` are views of ``packed`` (uint8), so one copy brings both to the host;
    ``workspace`` is the launch's scratch.  Pass a result back as ``out=`` to launch again into the same buffers."""
    result: torch.Tensor
    flags: torch.Tensor
    ap: Optional[torch.Tensor]
    valid: Optional[torch.Tensor]
    packed: torch.Tensor
    workspace: Optional[torch.Tensor]


def _packed(device, packed: Optional[torch.Tensor] = None):
    if packed is None:
        packed = torch.zeros(_PACKED_BYTES, dtype=torch.uint8, device=device)
    return packed, packed[:16].view(torch.float64), packed[16:20].view(torch.int32)


def metric_buffers(metric: str, G: int, C: int, device, packed: Optional[torch.Tensor] = None) -> MetricResult:
    """Outputs and workspace of ``metric`` ("ap" / "mae" on ``[G, C]`` inputs; "accuracy" / "f1_macro" on ``[G]``
    class indices and ``[G, C]`` scores), allocated once (``packed``: a uint8 buffer of at least 32 bytes whose head
    receives result and flags)."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    packed, result, flags = _packed(device, packed)
    if metric == "mae":
        return MetricResult(result, flags, None, None, packed, None)
    if metric in CLASS_METRICS:
        return MetricResult(result, flags, torch.zeros(C, dtype=torch.float64, device=device),
                            torch.zeros(C, C, dtype=torch.int32, device=device), packed, None)
    nbytes = int(_hip.lib().hscn_average_precision_workspace_bytes(G, C))
    return MetricResult(result, flags, torch.zeros(C, dtype=torch.float64, device=device),
                        torch.zeros(C, dtype=torch.int32, device=device), packed,
                        torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=device))


def _inputs(y_true: torch.Tensor, y_pred: torch.Tensor):
    if y_true.dim() != 2 or y_true.shape != y_pred.shape or y_true.numel() == 0:
        raise ValueError("y_true and y_pred must be non-empty [G, C] tensors of one shape")
    _hip.ptr(y_true), _hip.ptr(y_pred)            # (CPU tensors: the package's no-CPU-fallback error, before any cast)
    return (y_true.detach().to(torch.float32).contiguous(), y_pred.detach().to(torch.float32).contiguous(),
            int(y_true.size(0)), int(y_true.size(1)))


def average_precision_launch(y_true: torch.Tensor, y_pred: torch.Tensor,
                             out: Optional[MetricResult] = None) -> MetricResult:
    """Issue ``hscn_average_precision`` on ``[G, C]`` device tensors; nothing is read back."""
    y_true, y_pred, G, C = _inputs(y_true, y_pred)
    if out is None:
        out = metric_buffers("ap", G, C, y_true.device)
    nbytes = int(_hip.lib().hscn_average_precision_workspace_bytes(G, C))
    if out.ap.numel() != C or out.workspace.numel() < nbytes:
        raise ValueError("out= was allocated for another shape")
    _hip.call("hscn_average_precision", _hip.ptr(y_true), _hip.ptr(y_pred), G, C, _hip.ptr(out.ap), _hip.ptr(out.valid),
              _hip.ptr(out.result), _hip.ptr(out.flags), _hip.ptr(out.workspace), out.workspace.numel(), _hip.stream())
    return out


def mean_absolute_error_launch(y_true: torch.Tensor, y_pred: torch.Tensor,
                               out: Optional[MetricResult] = None) -> MetricResult:
    """Issue ``hscn_mean_absolute_error`` on ``[G, C]`` device tensors; nothing is read back."""
    y_true, y_pred, G, C = _inputs(y_true, y_pred)
    if out is None:
        out = metric_buffers("mae", G, C, y_true.device)
    _hip.call("hscn_mean_absolute_error", _hip.ptr(y_true), _hip.ptr(y_pred), G, C, _hip.ptr(out.result),
              _hip.ptr(out.flags), _hip.stream())
    return out


def multiclass_metrics_launch(y_true: torch.Tensor, y_pred: torch.Tensor,
                              out: Optional[MetricResult] = None) -> MetricResult:
    """Issue ``hscn_multiclass_metrics`` on ``y_true`` [G] int64 / ``y_pred`` [G, C] device tensors; nothing is read
    back.  ``out.result`` = (accuracy, macro-F1), ``out.ap`` the per-class F1, ``out.valid`` the confusion matrix."""
    if y_true.dim() != 1 or y_pred.dim() != 2 or y_true.size(0) != y_pred.size(0) or y_pred.numel() == 0:
        raise ValueError("y_true must be [G] class indices and y_pred non-empty [G, C] scores")
    if not (y_true.is_cuda and y_pred.is_cuda):   # (the package's no-CPU-fallback error, before any cast or copy)
        _hip.ptr(y_true if not y_true.is_cuda else y_pred)
    if y_true.dtype.is_floating_point or y_true.dtype == torch.bool:
        raise TypeError("y_true must hold integer class indices")
    y_true = y_true.detach().to(torch.int64).contiguous()
    y_pred = y_pred.detach().to(torch.float32).contiguous()
    G, C = int(y_pred.size(0)), int(y_pred.size(1))
    if out is None:
        out = metric_buffers("accuracy", G, C, y_true.device)
    if out.ap is None or out.ap.numel() != C or out.valid is None or tuple(out.valid.shape) != (C, C):
        raise ValueError("out= was allocated for another shape")
    _hip.call("hscn_multiclass_metrics", _hip.ptr(y_true), _hip.ptr(y_pred), G, C, _hip.ptr(out.valid),
              _hip.ptr(out.result), _hip.ptr(out.ap), _hip.ptr(out.flags), _hip.stream())
    return out


def metric_launch(metric: str):
    """The launch function of ``metric``: ``launch(y_true, y_pred, out=...)``."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return {"ap": average_precision_launch, "mae": mean_absolute_error_launch}.get(metric, multiclass_metrics_launch)


def result_index(metric: str) -> int:
    """Which word of a launch's ``result`` is ``metric`` (macro-F1 is the second word of the class-index launch)."""
    return 1 if metric == "f1_macro" else 0


def metric_value(metric: str, result: float, flags: int) -> float:
    """The reference's error behaviour on a metric launch's ``result[result_index(metric)]`` and ``flags[0]`` once they
    are on the host (the class-index metrics: scikit-learn's NaN check, torch's error for a class index outside
    ``[0, C)``)."""
    if metric in CLASS_METRICS:
        if flags & TARGET_OUT_OF_RANGE:
            raise IndexError("Target out of bounds: a class index outside [0, C)")
        if flags & NAN_INPUT:
            raise ValueError("Input contains NaN.")
        return float(result)
    if metric == "ap":
        if flags & NO_VALID_CLASS:
            raise RuntimeError("No positively labeled data available. Cannot compute Average"
                               "Precision.")
        if flags & NAN_INPUT:
            raise ValueError("Input contains NaN.")             # (sklearn's check of y_score)
    elif flags & NAN_INPUT:
        raise Exception("Model is predicting NaN.")
    return float(result)


def read_packed(packed: torch.Tensor):
    """ONE synchronising copy of a packed buffer: (float64 words, int32 words) on the host."""
    host = packed.cpu()
    return host[:16].view(torch.float64), host[16:].view(torch.int32)


def eval_ap_hip(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """``eval_ap`` through one HIP launch pair and one read-back."""
    f64, i32 = read_packed(average_precision_launch(y_true, y_pred).packed)
    return metric_value("ap", float(f64[0]), int(i32[0]))


def eval_mae_hip(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """``eval_mae`` through one HIP launch and one read-back."""
    f64, i32 = read_packed(mean_absolute_error_launch(y_true, y_pred).packed)
    return metric_value("mae", float(f64[0]), int(i32[0]))


def eval_accuracy_hip(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """``eval_accuracy`` through the HIP launches and one read-back."""
    f64, i32 = read_packed(multiclass_metrics_launch(y_true, y_pred).packed)
    return metric_value("accuracy", float(f64[0]), int(i32[0]))


def eval_f1_macro_hip(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """``eval_f1_macro`` through the HIP launches and one read-back."""
    f64, i32 = read_packed(multiclass_metrics_launch(y_true, y_pred).packed)
    return metric_value("f1_macro", float(f64[1]), int(i32[0]))


def eval_hip(metric: str):
    """``eval_<metric>_hip``."""
    return {"ap": eval_ap_hip, "mae": eval_mae_hip, "accuracy": eval_accuracy_hip, "f1_macro": eval_f1_macro_hip}[metric]
