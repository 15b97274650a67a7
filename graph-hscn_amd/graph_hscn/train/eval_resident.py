"""Evaluation of a split that lives in HBM (extension; the reference's evaluation is train/train.py:109-144,
mirrored as ``train.eval_epoch``).

``eval_epoch`` walks a host loader: every batch is collated in Python and copied to the device, every time, although
the validation and test splits never change and are never shuffled, and the epoch metric then loops over the classes
on the host.  ``DeviceEvaluator`` puts the split into a device dataset once; an evaluation is, per batch, one gather
launch on a precomputed id slice, the model's forward-only resident launch and ``hscn_criterion_fwd``, then the mean
of the per-batch losses and ONE metric launch (``metrics.average_precision_launch`` /
``mean_absolute_error_launch``).  ``run()`` reads nothing back; ``evaluate()`` reads 32 bytes once.

Same numbers as ``eval_epoch`` over an in-order loader of the same graphs and batch size: the batches are the same
(the gather is bit for bit the host collation), the launches are the same, the loss is the same unweighted float32
mean over the batches, the last, shorter one included (the reference's loader keeps it, loader/hetero_data.py:96-104).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from ..loss import criterion
from ..loss import raise_for_class_flags, class_target_flags
from ..metrics import (CLASS_METRICS, METRICS, MetricResult, metric_buffers, metric_launch, metric_value, read_packed,
                       result_index)
from . import batching

_GATHER_FAULT = 8      # loader.device_dataset: a graph id outside the dataset / a batch beyond the static capacity


class EvalRun(NamedTuple):
    """Device tensors of one evaluation: ``loss`` 0-dim float32 (mean of ``loss_log``), ``loss_log`` [num_batches],
    ``scores`` / ``targets`` [G, C] in dataset order (class-index targets: ``targets`` int64 [G], ``scores`` the
    log-probabilities), ``metric`` the metric launch's ``MetricResult`` (or ``None``)."""
    loss: torch.Tensor
    loss_log: torch.Tensor
    scores: torch.Tensor
    targets: torch.Tensor
    metric: Optional[MetricResult]


class DeviceEvaluator:
    """``graphs``: the split (``HeteroData`` for HSCN, ``Data`` for the MPNN baseline -- chosen as ``fit_resident``
    chooses); ``metric``: "ap", "mae", or -- for a split with class-index targets (HSCN only; C is the width of the
    model's head) -- "accuracy" / "f1_macro", or ``None`` (no metric launch, ``evaluate`` answers NaN for it).  A class
    index outside ``[0, C)`` is an ``IndexError`` of ``evaluate()``: the criterion's flag word comes over in the same
    copy."""

    def __init__(self, graphs: Sequence, model, loss_fn: str, batch_size: int, metric: Optional[str] = None):
        if metric not in METRICS + (None,):
            raise ValueError(f"metric must be one of {METRICS} or None, got {metric!r}")
        batching.refuse_layered_only(model, "DeviceEvaluator")
        batching.refuse_node_level(model, "DeviceEvaluator")
        batching.refuse_link_level(model, "DeviceEvaluator")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("DeviceEvaluator runs on the MI355X HIP path: move the model to 'cuda'")
        G = len(graphs)
        if G < 1:
            raise ValueError("empty split")
        self.model, self.loss_fn, self.metric = model, loss_fn, metric
        self.num_graphs, self.batch_size = G, int(batch_size)
        B = self.batch_size
        self.steps, self.tail = G // B, G % B      # (a split smaller than one batch is its own tail)
        self.num_batches = self.steps + (1 if self.tail else 0)
        self.ds = None
        if self.steps:
            self.ds = batching.dataset_class(model)(graphs, dev, B)
            ids = torch.arange(self.steps * B, dtype=torch.int64, device=dev)
            self.ids = [ids[i * B:(i + 1) * B] for i in range(self.steps)]
        # (the tail: collated once, kept on the device)
        self.tail_batch = batching.collate(model, list(graphs[self.steps * B:]), dev) if self.tail else None
        y0 = batching.targets(model, self.tail_batch if self.tail else self.ds.static.batch)
        self.class_index = batching.class_index_targets(y0)
        if metric is not None and (metric in CLASS_METRICS) != self.class_index:
            raise ValueError(f"metric {metric!r} does not fit the split's targets ('accuracy' / 'f1_macro' take class "
                             "indices, 'ap' / 'mae' [G, C] targets)")
        C = self.C = batching.score_width(model, y0)
        f32 = dict(dtype=torch.float32, device=dev)
        self.scores = torch.zeros(G, C, **f32)
        self.targets = torch.zeros(G, dtype=torch.int64, device=dev) if self.class_index else torch.zeros(G, C, **f32)
        self._class_flags = class_target_flags(dev) if self.class_index else None
        self.loss_log = torch.zeros(self.num_batches, **f32)
        # result [2] f64 | metric flags i32 | mean loss f32 | gather flag i32 | class-target flags i32: what evaluate()
        # reads, once
        self.packed = torch.zeros(32, dtype=torch.uint8, device=dev)
        self._loss = self.packed[20:24].view(torch.float32)
        self._gather_flag = self.packed[24:28].view(torch.int32)
        self._target_flag = self.packed[28:32].view(torch.int32)
        self.out = metric_buffers(metric, G, C, dev, self.packed) if metric else None

    def _batch(self, batch, lo: int, hi: int, i: int) -> None:
        pred, true = batching.forward(self.model, batch)
        loss, score = criterion(self.loss_fn, pred, true)
        self.loss_log[i].copy_(loss)
        self.scores[lo:hi].copy_(score)
        self.targets[lo:hi].copy_(true)

    @torch.no_grad()
    def run(self) -> EvalRun:
        """One evaluation of the split, enqueued on the current stream; no read-back."""
        model, B = self.model, self.batch_size
        was_training, engine = model.training, model.engine
        model.eval()
        model.engine = "resident"
        try:
            for i in range(self.steps):
                self._batch(self.ds.gather(self.ids[i]), i * B, (i + 1) * B, i)
            if self.tail:
                self._batch(self.tail_batch, self.steps * B, self.num_graphs, self.steps)
        finally:
            model.engine = engine
            model.train(was_training)
        self._loss.copy_(self.loss_log.mean())          # float32, unweighted over the batches: eval_epoch's definition
        if self.ds is not None:
            self._gather_flag.copy_(self.ds.flag)
        if self._class_flags is not None:
            self._target_flag.copy_(self._class_flags)
        if self.metric is not None:
            metric_launch(self.metric)(self.targets, self.scores, out=self.out)
        return EvalRun(self._loss.view(()), self.loss_log, self.scores, self.targets, self.out)

    def evaluate(self) -> Tuple[float, float]:
        """``(mean loss, metric)`` as ``train.eval_epoch`` returns them: ``run()``, then ONE synchronising copy that
        brings the loss, the metric, its flags and the dataset's gather flag (what ``ds.check()`` tests) together."""
        self.run()
        f64, i32 = read_packed(self.packed)
        if int(i32[2]) & _GATHER_FAULT:
            raise IndexError("a graph id was outside the dataset (or a batch exceeded the static capacity)")
        if int(i32[3]):
            self._class_flags.zero_()
            raise_for_class_flags(int(i32[3]))
        loss = float(i32[1:2].view(torch.float32)[0])
        perf = metric_value(self.metric, float(f64[result_index(self.metric)]), int(i32[0])) if self.metric \
            else float("nan")
        return loss, perf
