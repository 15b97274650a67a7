"""Epoch metrics of the training loop (reference graph_hscn/metrics.py:6-36), computed where the
tensors live: the reference moves every epoch's `[N, C]` labels and scores to the host and loops
over classes in sklearn; here the sort / cumulative sums run on the device (plain torch ops, they
are not on the hot path) and one scalar comes back.  Same definitions and error behaviour:
``eval_ap`` = mean over the classes that have both a positive and a negative label of sklearn's
``average_precision_score`` (step-wise integral of the precision-recall curve over distinct score
thresholds, NaN labels ignored); ``eval_mae`` = mean absolute error, raising on NaN predictions."""
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


# ---- the same two metrics as HIP launches (csrc/metrics.hip; include/hscn.h) ------------------------------------------
# ``eval_ap`` / ``eval_mae`` above read back per class; these sort and scan every class in one launch and the host
# reads ``result`` and ``flags`` once, together.

NO_VALID_CLASS, NAN_INPUT = 1, 2       # bits of ``flags`` (include/hscn.h)
_PACKED_BYTES = 32                     # result [2] f64 | flags [1] i32 | 3 spare 32-bit words, ONE buffer = one copy


class MetricResult(NamedTuple):
    """Device tensors of a metric launch.  ``result`` [2] float64 = (the metric, the number of valid classes -- for
    the MAE the element count), ``flags`` [1] int32; ``ap`` [C] float64 and ``valid`` [C] int32 per class (``None`` for
    the MAE).  ``result`` and ``flags`` are views of ``packed`` (uint8), so one copy brings both to the host;
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
    """Outputs and workspace of ``metric`` ("ap" / "mae") on ``[G, C]`` inputs, allocated once (``packed``: a uint8
    buffer of at least 32 bytes whose head receives result and flags)."""
    if metric not in ("ap", "mae"):
        raise ValueError(f"metric must be 'ap' or 'mae', got {metric!r}")
    packed, result, flags = _packed(device, packed)
    if metric == "mae":
        return MetricResult(result, flags, None, None, packed, None)
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


def metric_value(metric: str, result: float, flags: int) -> float:
    """The reference's error behaviour on a metric launch's ``result[0]`` and ``flags[0]`` once they are on the host."""
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
