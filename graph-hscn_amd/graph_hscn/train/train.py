"""Stage C training loop with the reference's structure
(/root/reference/graph_hscn/train/train.py:54-214): epoch loop, gradient
accumulation, optional clipping, eval + early stopping.  Differences: wandb is
optional, ``loss.item()`` is read once per epoch instead of once per iteration
(train.py:85 syncs the device every step), and an optional
``FlatGradReducer`` all-reduces gradients on stepping iterations only."""
from __future__ import annotations

import time
from typing import Callable, Optional

import torch
import torch.nn as nn

from ..config.config import OPTIM_DICT
from ..loss import criterion
from . import batching


def is_eval_epoch(epoch: int, max_epochs: int, eval_period: int) -> bool:  # train/utils.py:1-6
    return (epoch + 1) % eval_period == 0 or epoch == 0 or (epoch + 1) == max_epochs


def get_each_data_from_batch(data_list: list) -> list:  # train/utils.py:9-14
    """The graphs of a list of batches, in order."""
    out = []
    for batch in data_list:
        out.extend(batch.to_data_list())
    return out


def compute_posenc(loaders, data_cfg, num_features: int, pe_cfg, logger=None, device=None, *, stats=None,
                   is_undirected: bool = True):  # train/train.py:29-51
    """The positional-encoding stage in front of stage A: ONE ``SignNetNodeEncoder(pe_cfg, num_features,
    pe_cfg.dim_emb)`` with its random initial weights (the reference never trains it) runs under ``no_grad`` over
    every batch of every loader and replaces ``x`` by ``[linear_x(x) | pe]`` of width ``pe_cfg.dim_emb``.  Returns
    ``(new_loaders, batches)``: ``batches`` is the flat list of encoded batches in loader order
    (``get_each_data_from_batch`` turns it into graphs), and ``new_loaders[i]`` serves the encoded graphs of loader
    ``i`` in batches of ``data_cfg.batch_size``, loader 0 shuffled and the others in order.

    The encoder lives on ``device`` (default: "cuda" when available) and every batch is moved there; its engine is
    "auto", so a qualifying batch takes the one-launch kernel (include/hscn.h: hscn_signnet_encode).  The encoder is
    kept as ``compute_posenc.last_encoder`` for inspection.

    ``stats="device"``: a batch that arrives without ``eigvecs_sn`` gets its Laplacian statistics from
    ``transform.compute_posenc_stats_device`` (``pe_cfg``'s Laplacian and normaliser settings, ``is_undirected`` as the
    reference's loader passes it) on the encoder's device right before the encoder runs -- the PE stage of a batch is
    then two launches with no host pre-processing.  ``stats=None`` (default): the graphs carry pre-computed
    statistics, as in the reference.

    A ``config.RWSEConfig`` as ``pe_cfg`` selects the random-walk structural encoding instead: the encoder is ONE
    ``RWSENodeEncoder(pe_cfg, num_features, pe_cfg.dim_emb)``, and a batch that arrives without ``rwse`` gets it from
    ``transform.compute_rwse_stats_device`` right before the encoder runs, under ``stats=None`` and ``stats="device"``
    alike (there is no precomputed-only mode: the statistics are one cheap launch).  Everything else is the same.

    A ``config.LapPEConfig`` selects the Laplacian positional encoding with the DeepSet model: ONE
    ``LapPENodeEncoder(pe_cfg, num_features, pe_cfg.dim_emb)`` in eval mode (a frozen pre-stage flips no signs), and a
    batch without ``eigvecs_sn`` gets its statistics from ``transform.compute_posenc_stats_device`` under ``stats=None``
    and ``stats="device"`` alike.  (The trainable form is the models' own ``pos_enc``: model/_common.py.)"""
    if stats not in (None, "device"):
        raise ValueError(f"stats must be None or 'device', got {stats!r}")
    from ..config.config import LapPEConfig, RWSEConfig
    from ..data import DataLoader
    from ..encoder.signnet import SignNetNodeEncoder
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    rwse = isinstance(pe_cfg, RWSEConfig)
    lappe = isinstance(pe_cfg, LapPEConfig)
    if rwse:
        from ..encoder.rwse import RWSENodeEncoder
        from ..transform.rwse import compute_rwse_stats_device
        enc = RWSENodeEncoder(pe_cfg, num_features, pe_cfg.dim_emb).to(device)
    elif lappe:
        from ..encoder.lappe import LapPENodeEncoder
        enc = LapPENodeEncoder(pe_cfg, num_features, pe_cfg.dim_emb).to(device)
        enc.eval()                                 # a frozen pre-stage: no sign flips
    else:
        enc = SignNetNodeEncoder(pe_cfg, num_features, pe_cfg.dim_emb).to(device)
        enc.engine = "auto"
    compute_posenc.last_encoder = enc
    if logger is not None:
        logger.info("Running PE for each loader...")
    loaders_new, flat = [], []
    with torch.no_grad():
        for i, loader in enumerate(loaders):
            data_list = []
            for batch in loader:
                batch = batch.to(device)
                batch.x = batch.x.float()
                if rwse:
                    if getattr(batch, "rwse", None) is None:
                        compute_rwse_stats_device(batch, is_undirected, pe_cfg)
                elif (lappe or stats == "device") and getattr(batch, "eigvecs_sn", None) is None:
                    from ..transform.posenc import compute_posenc_stats_device
                    compute_posenc_stats_device(batch, is_undirected, pe_cfg)
                data_list.append(enc(batch))
            loaders_new.append(DataLoader(get_each_data_from_batch(data_list), batch_size=data_cfg.batch_size,
                                          shuffle=(i == 0)))
            flat.extend(data_list)
    return loaders_new, flat


def _link_metric_of(training_cfg) -> str:
    """The ranking metric a link-level model reports under ``training_cfg`` ("mrr" unless it names another)."""
    from ..metrics import LINK_METRICS
    metric = getattr(training_cfg, "metric", None)
    return metric if metric in LINK_METRICS else "mrr"


class EarlyStopping:
    """The evaluation block of the epoch loops (train/train.py:196-211).  ``update(validation loss, epoch)`` is true
    once the loss has not improved on its best by more than ``min_delta`` for ``patience`` evaluations in a row --
    except on the last epoch, which ends the run anyway.  With a ``reducer`` of several ranks they first agree on the
    mean of their losses (on ``device``): every rank must decide alike, or the next collective hangs."""

    def __init__(self, training_cfg, reducer=None, device=None):
        self.cfg, self.reducer, self.device = training_cfg, reducer, device
        self.best, self.stale = float("inf"), 0

    def update(self, loss: float, epoch: int) -> bool:
        if self.reducer is not None and self.reducer.world_size > 1:
            import torch.distributed as dist
            t = torch.tensor([loss], dtype=torch.float64, device=self.device)
            dist.all_reduce(t, group=self.reducer.group)
            loss = float(t.item()) / self.reducer.world_size
        if loss < self.best - self.cfg.min_delta:
            self.best, self.stale = loss, 0
        else:
            self.stale += 1
        return self.stale >= self.cfg.patience and epoch != self.cfg.epochs - 1

    def evaluate(self, epoch: int, logger, model, sources, metric_fn, eval_history: Optional[list] = None) -> bool:
        """Evaluate ``sources`` = (validation, test): host loaders through ``eval_epoch``, or
        ``eval_resident.DeviceEvaluator``s.  Whether to stop."""
        for split, source in zip(["Validation", "Test"], sources):
            if hasattr(source, "evaluate"):
                loss, perf = source.evaluate()
                if metric_fn is not None:
                    perf = metric_fn(source.targets, source.scores)
                if logger is not None:
                    logger.info(f"epoch {epoch} {split} loss {loss:.5f} perf {perf:.5f}")
            else:
                # (the keyword travels with a link-level model only: every other call is what it was)
                extra = {"link_metric": _link_metric_of(self.cfg)} if batching.link_level(model) else {}
                loss, perf = eval_epoch(epoch, logger, source, model, self.cfg.loss_fn, metric_fn, split, **extra)
            if eval_history is not None:
                eval_history.append((epoch, split, loss, perf))
            if split == "Validation" and self.update(loss, epoch):
                if logger is not None:
                    logger.info("stopping early")
                return True
        return False


def _link_ranks(model, metric_fn, link_metric):
    """``(accumulator, name)`` for a link-level model, ``(None, None)`` for any other.  A per-graph rank is not a
    function of concatenated targets and scores, so ``metric_fn(true, score)`` cannot express it and must be None for
    such a model: the epoch functions read ``link_metric`` ("mrr" / "hits@1" / "hits@3" / "hits@10"; None = "mrr")
    off a ``metrics.LinkRankAccumulator`` fed with the model's embeddings."""
    if not batching.link_level(model):
        if link_metric is not None:
            raise ValueError("link_metric belongs to a link-level model (task_level='link')")
        return None, None
    from ..metrics import LINK_METRICS, LinkRankAccumulator
    if metric_fn is not None:
        raise ValueError("a link-level model is scored per graph: pass link_metric=, not metric_fn")
    name = "mrr" if link_metric is None else link_metric
    if name not in LINK_METRICS:
        raise ValueError(f"a link-level model is scored by one of {LINK_METRICS}, not {link_metric!r}")
    return LinkRankAccumulator(), name


def _forward(model, batch, ranks):
    """``(pred, targets)`` of one batch; a link-level model's embeddings go to the epoch's accumulator."""
    if ranks is None:
        return batching.forward(model, batch)
    scores, labels, z = batching.link_forward(model, batch)
    ranks.update(z, batch)
    return scores, labels


def _link_result(ranks, name, device) -> float:
    """The epoch's ranking metric (one host copy), after the check of the pair decoder's own flag word."""
    from ..nn.head import check_pair_ids
    check_pair_ids(device)
    return ranks.result()[name]


def train_epoch(epoch, logger, loader, model, optimizer, loss_fn: str, metric_fn: Optional[Callable],
                batch_accumulation: int, clip_grad_norm: bool, reducer=None, link_metric: Optional[str] = None):
    """``link_metric``: the ranking metric a link-level model reports (``_link_ranks``)."""
    start = time.time()
    ranks, rank_name = _link_ranks(model, metric_fn, link_metric)
    model.train()
    optimizer.zero_grad()
    device = next(model.parameters()).device
    losses, y_true, y_pred = [], [], []
    num = len(loader)
    for it, batch in enumerate(loader):
        # train.py:78-80 leaves the batch where the loader put it; the HIP operators take device tensors only
        batch = batching.to_device(model, batch, device)
        pred, true = _forward(model, batch, ranks)
        loss, score = criterion(loss_fn, pred, true)
        if ranks is None:
            y_true.append(true)
            y_pred.append(score.detach())
        losses.append(loss.detach())
        loss.backward()
        if (it + 1) % batch_accumulation == 0 or it + 1 == num:
            if reducer is not None:
                reducer.reduce(float(pred.size(0)))
            if clip_grad_norm:
                nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            optimizer.step()
            optimizer.zero_grad()
    mean_loss = float(torch.stack(losses).mean().item())
    if hasattr(model, "check_flags"):              # (model/gps.py GPS: the attention launches' flag word)
        model.check_flags()
    if ranks is not None:
        perf = _link_result(ranks, rank_name, device)
    else:
        perf = metric_fn(torch.cat(y_true), torch.cat(y_pred)) if metric_fn else float("nan")
    if logger is not None:
        logger.info(f"epoch {epoch} train loss {mean_loss:.5f} perf {perf:.5f} ({time.time() - start:.2f}s)")
    return mean_loss, perf


@torch.no_grad()
def eval_epoch(epoch, logger, loader, model, loss_fn: str, metric_fn: Optional[Callable], split: str,
               link_metric: Optional[str] = None):
    model.eval()
    device = next(model.parameters()).device
    ranks, rank_name = _link_ranks(model, metric_fn, link_metric)
    losses, y_true, y_pred = [], [], []
    for batch in loader:
        batch = batching.to_device(model, batch, device)
        pred, true = _forward(model, batch, ranks)
        loss, score = criterion(loss_fn, pred, true)
        if ranks is None:
            y_true.append(true)
            y_pred.append(score)
        losses.append(loss)
    mean_loss = float(torch.stack(losses).mean().item())
    if hasattr(model, "check_flags"):              # (model/gps.py GPS: the attention launches' flag word)
        model.check_flags()
    if ranks is not None:
        perf = _link_result(ranks, rank_name, device)
    else:
        perf = metric_fn(torch.cat(y_true), torch.cat(y_pred)) if metric_fn else float("nan")
    if logger is not None:
        logger.info(f"epoch {epoch} {split} loss {mean_loss:.5f} perf {perf:.5f}")
    return mean_loss, perf


def train(logger, optim_cfg, training_cfg, loaders, model, metric_fn: Optional[Callable] = None, reducer=None):
    if getattr(optim_cfg, "scheduler", None) is not None:      # (the reference's loop has a constant rate)
        raise ValueError("OptimConfig.scheduler runs inside the one-launch optimizers: use train_resident.fit_resident")
    optimizer = OPTIM_DICT[optim_cfg.optim_type](lr=optim_cfg.lr, weight_decay=optim_cfg.weight_decay,
                                                 params=model.parameters())
    extra = {"link_metric": _link_metric_of(training_cfg)} if batching.link_level(model) else {}
    stopper = EarlyStopping(training_cfg)
    history = []
    for epoch in range(training_cfg.epochs):
        history.append(train_epoch(epoch, logger, loaders[0], model, optimizer, training_cfg.loss_fn, metric_fn,
                                   optim_cfg.batch_accumulation, optim_cfg.clip_grad_norm, reducer, **extra))
        if is_eval_epoch(epoch, training_cfg.epochs, training_cfg.eval_period) and \
                stopper.evaluate(epoch, logger, model, loaders[1:], metric_fn):
            break
    return history
