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


# ---- link-level ranking metrics: per-graph MRR and Hits@K (csrc/edge_head.hip; DESIGN.md sections 4 and 8) -------------------
# For every positive candidate pair (u, v) of a graph, its rank among the scores s(u, w) = <z_u, z_w> of the graph's
# other nodes w.  With g negatives scoring higher and e scoring equal, rank = 1 + g + e / 2 (the mean of the optimistic
# and the pessimistic rank); everything is kept as the integer rank2 = 2 g + e, so rank <= K is rank2 + 2 <= 2 K and
# the reciprocal rank is 2 / (rank2 + 2).  ``filter``: 0 = the negatives are all nodes w != v (u itself and u's other
# positive partners included); 1 = without the other positive partners of u ("filtered", the default of the
# evaluation entry points); 2 = additionally without u itself.

LINK_METRICS = ("mrr", "hits@1", "hits@3", "hits@10")
FILTERS = (0, 1, 2)
AVERAGINGS = ("graph", "pooled")
# bits of the launches' flag word (include/hscn.h: HSCN_PAIR_*)
PAIR_ID_OUT_OF_RANGE, PAIR_NAN_SCORE, PAIR_LABEL_NOT_BINARY, PAIR_BAD_SEGMENT, PAIR_NO_POSITIVE = 1, 2, 4, 8, 16
_LINK_PACKED_BYTES = 48                # result [4] f64 | flags [1] i32 | 3 spare 32-bit words, ONE buffer = one copy


def link_rank_counts(z: torch.Tensor, ptr: torch.Tensor, pair_ptr: torch.Tensor, pair_index: torch.Tensor,
                     edge_label: torch.Tensor, filter: int, score=None):
    """The restatement of ``hscn_pair_rank`` in plain torch ops: ``(rank2 [P] int32, per_graph [B, 5] float64)``.
    ``z`` [N, D] is used in float64 unless it is float32 (then the scores are float32 products summed by torch);
    ``ptr`` / ``pair_ptr`` [B + 1] node and pair ranges, ``pair_index`` [2, P] global node ids, ``edge_label`` [P].
    ``rank2`` is -1 for a pair that is not a ranked positive; ``per_graph[g]`` = (sum of reciprocal ranks in pair
    order, #rank <= 1, #rank <= 3, #rank <= 10, number of ranked positives).  A label outside {0, 1} is a
    ``ValueError``, a pair that leaves its graph an ``IndexError``; a positive whose own score is NaN is not ranked.
    ``score``: a function giving the [n, n] score matrix of a graph's rows ``z[nb:ne]`` in place of their product
    (scores evaluated elsewhere, say by ``nn.head.pair_dot``, ranked by the integer rules here)."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    z = z.detach()
    if z.dtype != torch.float32:
        z = z.to(torch.float64)
    edge_label = edge_label.detach()
    if not bool(((edge_label == 0) | (edge_label == 1)).all()):
        raise ValueError("edge_label must hold 0 or 1")
    dev = z.device
    B, P = int(ptr.numel()) - 1, int(pair_index.size(1))
    nodes, pairs = [int(v) for v in ptr.tolist()], [int(v) for v in pair_ptr.tolist()]
    rank2 = torch.full((P,), -1, dtype=torch.int32, device=dev)
    per_graph = torch.zeros(B, 5, dtype=torch.float64, device=dev)
    for g in range(B):
        nb, ne, pb, pe = nodes[g], nodes[g + 1], pairs[g], pairs[g + 1]
        n = ne - nb
        idx = pair_index[:, pb:pe]
        if idx.numel() and (int(idx.min()) < nb or int(idx.max()) >= ne):
            raise IndexError(f"a candidate pair of graph {g} leaves its node range [{nb}, {ne})")
        which = torch.nonzero(edge_label[pb:pe] == 1).flatten()
        if which.numel() == 0:
            continue
        U, V = idx[0, which] - nb, idx[1, which] - nb
        S = z[nb:ne] @ z[nb:ne].T if score is None else score(z[nb:ne]).to(dev)
        rows = S[U]                                                       # [positives, n]: s(u, .)
        k = torch.arange(which.numel(), device=dev)
        spos = rows[k, V].unsqueeze(1)
        neg = torch.ones(which.numel(), n, dtype=torch.bool, device=dev)
        if filter >= 1:
            positive = torch.zeros(n, n, dtype=torch.bool, device=dev)
            positive[U, V] = True
            neg &= ~positive[U]
        if filter == 2:
            neg[k, U] = False
        neg[k, V] = False
        gt = ((rows > spos) & neg).sum(1)
        eq = ((rows == spos) & neg).sum(1)
        r2 = (2 * gt + eq).to(torch.int32)
        ranked = ~torch.isnan(spos.squeeze(1))
        r2 = torch.where(ranked, r2, torch.full_like(r2, -1))
        rank2[pb + which] = r2
        total = 0.0
        for v in r2[ranked].tolist():                                     # in pair order, as the kernel adds them
            total += 2.0 / (v + 2)
        rr = r2[ranked].to(torch.int64) + 2
        per_graph[g] = torch.tensor([total, float((rr <= 2).sum()), float((rr <= 6).sum()), float((rr <= 20).sum()),
                                     float(ranked.sum())], dtype=torch.float64)
    return rank2, per_graph


def link_means(per_graph: torch.Tensor, averaging: str = "graph"):
    """(MRR, Hits@1, Hits@3, Hits@10) of a per-graph table.  "graph": per graph the mean over its positives, then the
    mean over the graphs that have at least one, in graph order; "pooled": one mean over all positives."""
    if averaging not in AVERAGINGS:
        raise ValueError(f"averaging must be one of {AVERAGINGS}, got {averaging!r}")
    sums, count = [0.0] * 4, 0
    for row in per_graph.tolist():
        if not row[4] > 0:
            continue                                                      # a graph without positives is left out
        for k in range(4):
            sums[k] += row[k] if averaging == "pooled" else row[k] / row[4]
        count += int(row[4]) if averaging == "pooled" else 1
    if count == 0:
        raise RuntimeError("No positive pair available. Cannot compute a ranking metric.")
    return tuple(s / count for s in sums)


def eval_link_ranks(z, ptr, pair_ptr, pair_index, edge_label, filter: int = 1, averaging: str = "graph"):
    """(MRR, Hits@1, Hits@3, Hits@10) through ``link_rank_counts``."""
    return link_means(link_rank_counts(z, ptr, pair_ptr, pair_index, edge_label, filter)[1], averaging)


class LinkRankResult(NamedTuple):
    """Device tensors of a ranking launch: ``rank2`` [P] int32, ``per_graph`` [B, 5] float64, and ``result`` [4]
    float64 (MRR, Hits@1, Hits@3, Hits@10) with ``flags`` [1] int32, both views of ``packed``: one copy brings them
    to the host."""
    rank2: Optional[torch.Tensor]
    per_graph: torch.Tensor
    result: torch.Tensor
    flags: torch.Tensor
    packed: torch.Tensor


def _link_packed(device, packed: Optional[torch.Tensor] = None):
    if packed is None:
        packed = torch.zeros(_LINK_PACKED_BYTES, dtype=torch.uint8, device=device)
    return packed, packed[:32].view(torch.float64), packed[32:36].view(torch.int32)


def pair_rank_supported(max_nodes: int, D: int) -> int:
    """0: refused; 1: a graph of ``max_nodes`` nodes is ranked from LDS; 2: from global memory (the same kernel)."""
    return int(_hip.lib().hscn_pair_rank_supported(int(max_nodes), int(D)))


def pair_rank_launch(z: torch.Tensor, ptr32: torch.Tensor, pair_ptr32: torch.Tensor, structure, filter: int = 1,
                     averaging: str = "graph", want_rank2: bool = True, packed: Optional[torch.Tensor] = None,
                     acc_sum: Optional[torch.Tensor] = None, acc_count: Optional[torch.Tensor] = None,
                     max_nodes: int = 0) -> LinkRankResult:
    """Issue ``hscn_pair_rank`` and ``hscn_pair_rank_reduce`` on device tensors; nothing is read back.  ``structure``:
    the batch's ``nn.head.PairStructure`` built with its labels; ``ptr32`` / ``pair_ptr32`` int32 [B + 1].
    ``acc_sum`` [4] float64 / ``acc_count`` [1] int64: an epoch's running totals (``LinkRankAccumulator``); the flag
    word of ``packed`` is ORed into, never cleared here (but for ``PAIR_NO_POSITIVE``, which a launch whose total
    holds a positive takes back).  ``max_nodes``: the batch's largest graph, which sizes the launch's LDS (0: the whole
    budget).  ``rank2`` is -1 wherever the kernel does not rank, pairs outside every graph's range included."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
    if averaging not in AVERAGINGS:
        raise ValueError(f"averaging must be one of {AVERAGINGS}, got {averaging!r}")
    if z.dim() != 2:
        raise ValueError("z must be [N, D]")
    _hip.ptr(z)                                        # (a CPU tensor: the package's no-CPU-fallback error)
    if structure.edge_label is None:
        raise ValueError("the PairStructure was built without labels")
    if not _hip.lib().hscn_pair_dot_supported(int(z.size(1))):
        raise RuntimeError(f"the ranking kernel takes an embedding width that is a multiple of 4 in [4, 64] "
                           f"(hscn_pair_rank_supported), not D={z.size(1)}")
    z = z.detach().to(torch.float32).contiguous()
    if z.data_ptr() % 16:
        z = z.clone()
    dev = z.device
    B, N, P = int(ptr32.numel()) - 1, int(z.size(0)), int(structure.num_pairs)
    ptr32 = ptr32.to(device=dev, dtype=torch.int32).contiguous()
    pair_ptr32 = pair_ptr32.to(device=dev, dtype=torch.int32).contiguous()
    packed, result, flags = _link_packed(dev, packed)
    rank2 = torch.full((P,), -1, dtype=torch.int32, device=dev) if want_rank2 else None
    per_graph = torch.empty(B, 5, dtype=torch.float64, device=dev)
    pos = structure.positives
    _hip.call("hscn_pair_rank", _hip.ptr(z), _hip.ptr(ptr32), _hip.ptr(pair_ptr32), _hip.ptr(structure.index32),
              _hip.ptr(structure.edge_label), _hip.ptr(pos.rowptr) if pos is not None else None,
              _hip.ptr(pos.eid) if pos is not None else None, B, N, P, int(z.size(1)), int(filter), int(max_nodes),
              _hip.ptr(rank2),
              _hip.ptr(per_graph), _hip.ptr(flags), _hip.stream())
    _hip.call("hscn_pair_rank_reduce", _hip.ptr(per_graph), B, AVERAGINGS.index(averaging), _hip.ptr(acc_sum),
              _hip.ptr(acc_count), _hip.ptr(result), _hip.ptr(flags), _hip.stream())
    return LinkRankResult(rank2, per_graph, result, flags, packed)


def link_metric_values(result, flags: int):
    """The four numbers of a ranking launch once ``result`` and ``flags`` are on the host, or the error its flags
    stand for."""
    if flags & (PAIR_ID_OUT_OF_RANGE | PAIR_BAD_SEGMENT):
        raise IndexError("a candidate pair leaves its graph's node range")
    if flags & PAIR_LABEL_NOT_BINARY:
        raise ValueError("edge_label must hold 0 or 1")
    if flags & PAIR_NAN_SCORE:
        raise ValueError("Input contains NaN.")
    if flags & PAIR_NO_POSITIVE:
        raise RuntimeError("No positive pair available. Cannot compute a ranking metric.")
    return tuple(float(v) for v in result[:4])


def read_link_packed(packed: torch.Tensor):
    """ONE synchronising copy of a ranking launch's packed buffer: (float64 [4], flags)."""
    host = packed.cpu()
    return host[:32].view(torch.float64), int(host[32:36].view(torch.int32)[0])


def eval_link_ranks_hip(z, ptr32, pair_ptr32, structure, filter: int = 1, averaging: str = "graph",
                        max_nodes: int = 0):
    """``eval_link_ranks`` through the HIP launches and one read-back."""
    f64, flags = read_link_packed(pair_rank_launch(z, ptr32, pair_ptr32, structure, filter, averaging,
                                                   want_rank2=False, max_nodes=max_nodes).packed)
    return link_metric_values(f64, flags)


class LinkRankAccumulator:
    """An epoch's ranking metric over several batches: every ``update`` launches on its batch and adds the batch's
    graphs to running float64 sums and an int64 count on the device; ``result()`` is the one host copy."""

    def __init__(self, filter: int = 1, averaging: str = "graph"):
        if filter not in FILTERS:
            raise ValueError(f"filter must be one of {FILTERS}, got {filter!r}")
        if averaging not in AVERAGINGS:
            raise ValueError(f"averaging must be one of {AVERAGINGS}, got {averaging!r}")
        self.filter, self.averaging = filter, averaging
        self.packed = self.acc_sum = self.acc_count = None

    def reset(self) -> None:
        for t in (self.packed, self.acc_sum, self.acc_count):
            if t is not None:
                t.zero_()

    def update(self, z: torch.Tensor, batch) -> None:
        """``z``: the model's [N, D] embeddings of ``batch`` (a ``Batch``, or a ``HeteroBatch`` whose local node type
        carries the pairs), on the device."""
        from .nn.head import PairStructure
        store = batch["local"] if hasattr(batch, "node_types") else batch
        if self.packed is None or self.packed.device != z.device:
            self.packed = torch.zeros(_LINK_PACKED_BYTES, dtype=torch.uint8, device=z.device)
            self.acc_sum = torch.zeros(4, dtype=torch.float64, device=z.device)
            self.acc_count = torch.zeros(1, dtype=torch.int64, device=z.device)
        pair_rank_launch(z, store.ptr32, store.pair_ptr32, PairStructure.of(store, z.size(0)), self.filter,
                         self.averaging, want_rank2=False, packed=self.packed, acc_sum=self.acc_sum,
                         acc_count=self.acc_count, max_nodes=int(store.max_nodes) if "max_nodes" in store else 0)

    def result(self) -> dict:
        """{"mrr", "hits@1", "hits@3", "hits@10"} of everything since the last ``reset`` (synchronising)."""
        if self.packed is None:
            raise RuntimeError("No positive pair available. Cannot compute a ranking metric.")
        f64, flags = read_link_packed(self.packed)
        return dict(zip(LINK_METRICS, link_metric_values(f64, flags)))
