"""Stage C training loop at the speed of the kernels (extension; the reference's loop is train/train.py:54-214,
mirrored in ``train.py`` next to this file).

Same schedule -- epochs of shuffled mini-batches, an optimizer step per batch, evaluation every ``eval_period``
epochs, early stopping on the validation loss -- but the training split lives in HBM
(``loader.device_dataset.DeviceHeteroDataset``), a step is "permutation slice -> one gather launch -> one replay of
the captured forward + loss + backward + optimizer step", and the host reads nothing back until the epoch ends.
The last, shorter batch of an epoch (the reference's loader keeps it, loader/hetero_data.py:96-104) runs through
the eager path on a host-collated batch with the same optimizer, so every graph is visited once per epoch.

``OptimConfig.batch_accumulation`` (k) and ``clip_grad_norm`` are honoured as train/train.py:89-95 honours them: the
optimizer steps on iterations with ``(it + 1) % k == 0 or it + 1 == num_batches`` (``optimizer_steps_at``) on the
gradients summed since the last step, clipped to norm 1 first.  With k > 1 two graphs are captured over the same
buffers: the micro-batch iteration (gather, then the step ADDING its gradients to the flat buffer) and the boundary
iteration (the same, then all-reduce, clip, optimizer step, gradients zeroed); with ``optim.FlatAdam`` the clip and
the zeroing ride on its one launch, so no iteration issues a launch it did not issue before.  All three members of
``OPTIM_DICT`` have such a launch (``optim.FlatAdagrad`` for Adagrad), and ``OptimConfig.scheduler`` is evaluated
inside it from the device step counter (``optim.LRSchedule``): the captured iteration stays one replay.
"""
from __future__ import annotations

import time
from types import SimpleNamespace
from typing import Callable, List, Optional, Sequence

import torch

from ..config.config import OPTIM_DICT
from ..loss import check_class_targets, criterion
from ..optim import FLAT_OPTIMIZERS, clip_grad_norm_flat, collect_autograd
from ..replay import CapturedStep
from . import batching
from . import train as _train

CLIP_MAX_NORM = 1.0     # train/train.py:92 (the reference's nn.utils.clip_grad_norm_(params, 1.0))


def optimizer_steps_at(it: int, num_batches: int, batch_accumulation: int) -> bool:
    """Whether iteration ``it`` (0-based) of an epoch of ``num_batches`` batches steps the optimizer: every
    ``batch_accumulation``-th batch and always the last one (train/train.py:89 -- ``train.train_epoch``)."""
    return (it + 1) % batch_accumulation == 0 or it + 1 == num_batches


def schedule_from_config(optim_cfg, epochs: int, num_batches: int, batch_accumulation: int):
    """``OptimConfig.scheduler`` (lengths in epochs) as an ``optim.LRSchedule`` in optimizer steps: an epoch of
    ``num_batches`` batches steps on the iterations ``optimizer_steps_at`` names.  None without a scheduler."""
    name = getattr(optim_cfg, "scheduler", None)
    if name is None:
        return None
    from ..optim import LRSchedule
    per_epoch = sum(optimizer_steps_at(i, num_batches, batch_accumulation) for i in range(num_batches))
    return LRSchedule(name, warmup_steps=optim_cfg.warmup_epochs * per_epoch, total_steps=epochs * per_epoch,
                      period=optim_cfg.step_epochs * per_epoch, gamma=optim_cfg.gamma,
                      min_factor=optim_cfg.min_lr_factor, base_lr=optim_cfg.lr)


def _make_optimizer(optim_cfg, model, flat: bool, clip: bool, acc: bool, schedule=None):
    """``(optimizer, capturable)``.  ``flat`` (optim.FlatAdam / FlatAdagrad: the update as ONE launch, clip, zeroing
    and ``schedule`` in it): a callable ``step -> optimizer`` for ``CapturedStep`` to build on the step's flat
    gradient buffer."""
    kw = dict(lr=optim_cfg.lr, weight_decay=optim_cfg.weight_decay)
    if flat:
        from ..optim import flat_optimizer_from_config
        fkw = dict(kw, max_norm=CLIP_MAX_NORM if clip else None, zero_grads=acc)
        if schedule is not None:
            fkw["schedule"] = schedule
        return (lambda st: flat_optimizer_from_config(optim_cfg.optim_type, st.param_grads, st.grads, **fkw)), True
    opt_cls = OPTIM_DICT[optim_cfg.optim_type]
    try:
        optimizer = opt_cls(model.parameters(), capturable=True, fused=True, **kw)
    except (TypeError, RuntimeError):          # (torch's Adagrad has neither switch: its step stays outside the graph)
        optimizer = opt_cls(model.parameters(), **kw)
    return optimizer, bool(optimizer.defaults.get("capturable", False))


def _boundary_outside_graph(run, weight: float) -> None:
    """What the graph does not hold at a stepping iteration (a non-capturable optimizer; the eager tail)."""
    if run.reducer is not None:
        run.reducer.reduce(weight, weight * run.reducer.world_size)
    if run.clip_norm is not None:              # (the one-launch optimizers clip and zero in their own launch)
        clip_grad_norm_flat(run.flat_grads, CLIP_MAX_NORM, run.clip_norm)
    run.optimizer.step()
    if run.acc and not run.flat:
        run.flat_grads.zero_()


def _captured_epoch(run, steps: int, num_batches: int, record) -> None:
    """The epoch's ``steps`` full batches: one replay each (next permutation slice + iteration)."""
    if not run.in_graph:
        run.step.bind_grads()                  # (the eager tail of the previous epoch re-pointed p.grad)
    B, y = run.ds.batch_size, batching.targets(run.model, run.ds.static.batch)
    for i in range(steps):
        stepping = optimizer_steps_at(i, num_batches, run.k)
        run.step.replay(step_optimizer=stepping)
        if stepping and not run.in_graph:
            _boundary_outside_graph(run, float(B))
        record(i, i * B, run.step.loss, run.step.score, y)


def _tail_step(run, graphs: Sequence, loss_fn: str, record, i: int, lo: int) -> None:
    """The epoch's last, shorter batch: host-collated, through autograd, the same optimizer.  It is the epoch's last
    iteration, so it steps (``optimizer_steps_at``)."""
    hb = batching.collate(run.model, graphs, run.ds.device)
    run.optimizer.zero_grad(set_to_none=True)
    pred, y = batching.forward(run.model, hb)
    loss, score = criterion(loss_fn, pred, y)
    loss.backward()
    # the window's earlier micro-batches are in the flat buffer: the tail's p.grad is added to them there (copied,
    # without accumulation) and p.grad points at the buffer again -- what the reducer and the optimizer take
    collect_autograd(run.step.grads, run.acc)
    run.step.bind_grads()
    _boundary_outside_graph(run, float(len(graphs)))
    record(i, lo, loss.detach(), score.detach(), y)


def fit_resident(logger, optim_cfg, training_cfg, train_graphs: Sequence, eval_loaders: Sequence, model,
                 batch_size: int, metric_fn: Optional[Callable] = None, seed: int = 0, reducer=None,
                 flat_optimizer: bool = True, epoch_orders: Optional[list] = None, *,
                 eval_graphs: Optional[Sequence] = None, metric: Optional[str] = None,
                 eval_history: Optional[list] = None, run_info: Optional[dict] = None) -> List[tuple]:
    """Returns ``[(mean train loss, train metric), ...]`` per epoch, like ``train.train``.  ``eval_loaders`` =
    ``[validation, test]`` loaders of host batches (evaluated with ``train.eval_epoch``).

    Data parallel: every rank calls this with ITS shard of the training graphs (``distributed.shard_list``; equal
    shard sizes, so that all ranks take the same number of steps) and a ``distributed.FlatGradReducer`` as
    ``reducer`` (built with ``equal_weights=True`` it averages with no scaling launch).
    The iteration stays ONE replay: forward + loss + backward, the RCCL all-reduce of the flat gradient buffer where
    the backward left it, the optimizer step -- all captured (an optimizer without a capturable step is stepped, and
    the collective issued, outside the graph).  The eager tail batch is reduced the same way.

    ``epoch_orders``: a list that receives every epoch's permutation of ``train_graphs`` as a host tensor (one
    read-back per epoch, only when a list is passed): batch i of the epoch is ``order[i * B:(i + 1) * B]``, the
    order ``train.train_epoch`` has to see to take the same steps.

    ``model`` may also be the MPNN baseline (``model.mpnn.MPNN``) with ``train_graphs`` a list of ``Data``: the
    dataset is then a ``DeviceGraphDataset`` (``[B, C]`` targets only: the MPNN's and the vl model's one-launch steps
    refuse class indices) and the captured step ``step.MPNNResidentTrainStep`` (one launch + the
    gradient fold; ``batching`` picks both); evaluation through ``train.eval_epoch`` takes the MPNN's forward-only
    launch.

    Evaluation on the device (keyword-only; the defaults leave the loop as it was): ``eval_graphs`` =
    ``(validation graphs, test graphs)`` puts the two splits into ``eval_resident.DeviceEvaluator``s built once before
    the first epoch -- no host loader, collation or copy per evaluation -- and ``eval_loaders`` may then be ``None``.
    ``metric`` = "ap" / "mae" (or, for class-index targets, "accuracy" / "f1_macro") computes the epoch metric, of the training split and of the evaluators, with the HIP
    launches of ``metrics`` (one read-back brings the loss and the metric together) in place of a ``metric_fn``;
    passing both is a ``ValueError``.  ``eval_history``: a list that receives ``(epoch, split, loss, perf)`` of every
    evaluation.

    ``optim_cfg.scheduler`` (with ``flat_optimizer=True`` only: torch's optimizers would need a host-side scheduler
    step between replays) becomes an ``optim.LRSchedule`` in optimizer steps (``schedule_from_config``), evaluated
    inside the optimizer's launch.  ``run_info``: a dict that receives ``optimizer``, ``flat``, ``in_graph`` (the whole
    stepping iteration is one graph) and ``schedule`` of the run."""
    if getattr(optim_cfg, "scheduler", None) is not None and not flat_optimizer:
        raise ValueError("a scheduler runs inside the one-launch optimizers: it needs flat_optimizer=True")
    if metric is not None and metric_fn is not None:        # (argument checks come before anything touches a device)
        raise ValueError("pass metric= (the HIP metric launch) or metric_fn=, not both")
    from .. import metrics as _metrics
    if metric not in _metrics.METRICS + (None,):
        raise ValueError(f"metric must be one of {_metrics.METRICS} or None, got {metric!r}")
    if eval_graphs is not None and len(eval_graphs) != 2:
        raise ValueError("eval_graphs is the pair (validation graphs, test graphs)")
    batching.refuse_layered_only(model, "fit_resident")
    batching.refuse_node_level(model, "fit_resident")
    batching.refuse_link_level(model, "fit_resident")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("fit_resident runs on the MI355X HIP path: move the model to 'cuda'")
    k = int(getattr(optim_cfg, "batch_accumulation", 1) or 1)
    if k < 1:
        raise ValueError("batch_accumulation must be at least 1")
    clip = bool(getattr(optim_cfg, "clip_grad_norm", False))
    acc = k > 1
    G, B = len(train_graphs), int(batch_size)
    if G < B:
        raise ValueError("fewer training graphs than one batch")
    loss_fn = training_cfg.loss_fn
    ds = batching.dataset_class(model)(train_graphs, dev, B)
    flat = flat_optimizer and optim_cfg.optim_type in FLAT_OPTIMIZERS
    if getattr(optim_cfg, "scheduler", None) is not None and not flat:
        raise ValueError(f"no one-launch optimizer for {optim_cfg.optim_type!r}: a scheduler cannot run")
    num_batches = G // B + (1 if G % B else 0)
    schedule = schedule_from_config(optim_cfg, training_cfg.epochs, num_batches, k)
    # in_graph: the whole iteration -- backward, gradient all-reduce (if any), optimizer step -- is one graph
    optimizer, in_graph = _make_optimizer(optim_cfg, model, flat, clip, acc, schedule)
    gen = torch.Generator(device=dev).manual_seed(seed)
    model.train()
    model.engine = "resident"
    ds.new_epoch(gen)
    # the gather of the next permutation slice is captured in front of the step: a replay = next batch + iteration
    step = CapturedStep(model, ds.static, loss_fn, optimizer=optimizer if in_graph else None,
                        pre=ds.gather_next, reducer=reducer if in_graph else None, accumulate=acc,
                        max_norm=CLIP_MAX_NORM if clip and in_graph and not flat else None)
    clip_norm = step.clip_norm             # the pre-clip norm of the clip launch: the one in the graph, or, with the
    if clip and not in_graph:              # optimizer outside it, _boundary_outside_graph's
        clip_norm = torch.zeros(1, dtype=torch.float32, device=dev)
    run = SimpleNamespace(model=model, ds=ds, step=step, optimizer=step.optimizer if flat else optimizer,
                          reducer=reducer, flat=flat, in_graph=in_graph, acc=acc, k=k, clip_norm=clip_norm,
                          flat_grads=step.step.grads[:step.step.P])     # every parameter gradient (not the loss column)

    if run_info is not None:
        run_info.update(optimizer=run.optimizer, flat=flat, in_graph=in_graph, schedule=schedule)

    steps, tail = G // B, G % B
    y_static = batching.targets(model, ds.static.batch)
    class_index = batching.class_index_targets(y_static)
    if metric is not None and (metric in _metrics.CLASS_METRICS) != class_index:
        raise ValueError(f"metric {metric!r} does not fit the targets ('accuracy' / 'f1_macro' take class indices, "
                         "'ap' / 'mae' [G, C] targets)")
    C = batching.score_width(model, y_static)
    loss_log = torch.zeros(num_batches, dtype=torch.float32, device=dev)
    want_metric = metric_fn is not None or metric is not None
    scores = torch.zeros(G, C, dtype=torch.float32, device=dev) if want_metric else None
    targets = None
    if want_metric:
        targets = torch.zeros(G, dtype=torch.int64, device=dev) if class_index else \
            torch.zeros(G, C, dtype=torch.float32, device=dev)

    def record(i: int, lo: int, loss, score, y) -> None:
        loss_log[i].copy_(loss)
        if want_metric:
            scores[lo:lo + score.size(0)].copy_(score)
            targets[lo:lo + y.size(0)].copy_(y)

    eval_metric_fn = metric_fn
    if metric is not None:
        train_metric = _metrics.metric_buffers(metric, G, C, dev)
        train_loss = train_metric.packed[20:24].view(torch.float32)     # beside result and flags: one read-back
        launch = _metrics.metric_launch(metric)
        eval_metric_fn = _metrics.eval_hip(metric)                      # (host loaders)
    eval_sources = eval_loaders or []
    if eval_graphs is not None:
        from .eval_resident import DeviceEvaluator
        eval_sources = [DeviceEvaluator(g, model, loss_fn, B, metric) for g in eval_graphs]
        eval_metric_fn = metric_fn              # (the evaluators compute ``metric`` themselves)
    stopper = _train.EarlyStopping(training_cfg, reducer, dev)
    history = []
    for epoch in range(training_cfg.epochs):
        start = time.time()
        model.train()
        perm = ds.new_epoch(gen)               # permutation + batch counter on the device
        if epoch_orders is not None:
            epoch_orders.append(perm.cpu())
        _captured_epoch(run, steps, num_batches, record)
        if tail:
            _tail_step(run, [train_graphs[j] for j in perm[steps * B:].tolist()], loss_fn, record, steps, steps * B)
        if metric is not None:
            launch(targets, scores, out=train_metric)
            train_loss.copy_(loss_log.mean())
            f64, i32 = _metrics.read_packed(train_metric.packed)      # the epoch's only read-back
            mean_loss = float(i32[1:2].view(torch.float32)[0])
            perf = _metrics.metric_value(metric, float(f64[_metrics.result_index(metric)]), int(i32[0]))
        else:
            mean_loss = float(loss_log.mean().item())                 # the epoch's only read-back
            perf = metric_fn(targets, scores) if metric_fn else float("nan")
        history.append((mean_loss, perf))
        if logger is not None:
            logger.info(f"epoch {epoch} train loss {mean_loss:.5f} perf {perf:.5f} ({time.time() - start:.2f}s)")
        if _train.is_eval_epoch(epoch, training_cfg.epochs, training_cfg.eval_period) and \
                stopper.evaluate(epoch, logger, model, eval_sources, eval_metric_fn, eval_history):
            break
    ds.check()
    if class_index:
        step.step.check()                      # (class indices outside [0, C): the captured step's flag word ...
        check_class_targets(dev)               # ... and the eager tail's, loss.class_target_flags)
    return history
