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
the zeroing ride on its one launch, so no iteration issues a launch it did not issue before.
"""
from __future__ import annotations

import time
from typing import Callable, List, Optional, Sequence

import torch

from ..config.config import OPTIM_DICT
from ..data import Batch, HeteroBatch, HeteroData
from ..loader.device_dataset import DeviceHeteroDataset
from ..loss import criterion
from ..optim import clip_grad_norm_flat
from ..replay import CapturedStep
from .train import eval_epoch, is_eval_epoch

CLIP_MAX_NORM = 1.0     # train/train.py:92 (the reference's nn.utils.clip_grad_norm_(params, 1.0))


def optimizer_steps_at(it: int, num_batches: int, batch_accumulation: int) -> bool:
    """Whether iteration ``it`` (0-based) of an epoch of ``num_batches`` batches steps the optimizer: every
    ``batch_accumulation``-th batch and always the last one (train/train.py:89 -- ``train.train_epoch``)."""
    return (it + 1) % batch_accumulation == 0 or it + 1 == num_batches


def fit_resident(logger, optim_cfg, training_cfg, train_graphs: Sequence, eval_loaders: Sequence, model,
                 batch_size: int, metric_fn: Optional[Callable] = None, seed: int = 0, reducer=None,
                 flat_optimizer: bool = True, epoch_orders: Optional[list] = None, *,
                 eval_graphs: Optional[Sequence] = None, metric: Optional[str] = None,
                 eval_history: Optional[list] = None) -> List[tuple]:
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
    dataset is then a ``DeviceGraphDataset`` and the captured step ``step.MPNNResidentTrainStep`` (one launch + the
    gradient fold); evaluation through ``train.eval_epoch`` takes the MPNN's forward-only launch.

    Evaluation on the device (keyword-only; the defaults leave the loop as it was): ``eval_graphs`` =
    ``(validation graphs, test graphs)`` puts the two splits into ``eval_resident.DeviceEvaluator``s built once before
    the first epoch -- no host loader, collation or copy per evaluation -- and ``eval_loaders`` may then be ``None``.
    ``metric`` = "ap" / "mae" computes the epoch metric, of the training split and of the evaluators, with the HIP
    launches of ``metrics`` (one read-back brings the loss and the metric together) in place of a ``metric_fn``;
    passing both is a ``ValueError``.  ``eval_history``: a list that receives ``(epoch, split, loss, perf)`` of every
    evaluation."""
    if metric is not None and metric_fn is not None:        # (argument checks come before anything touches a device)
        raise ValueError("pass metric= (the HIP metric launch) or metric_fn=, not both")
    if metric not in (None, "ap", "mae"):
        raise ValueError(f"metric must be 'ap', 'mae' or None, got {metric!r}")
    if eval_graphs is not None and len(eval_graphs) != 2:
        raise ValueError("eval_graphs is the pair (validation graphs, test graphs)")
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
    from ..model.mpnn import MPNN
    mpnn = isinstance(model, MPNN)      # the MPNN baseline on a list of Data: homogeneous device dataset, same loop
    if mpnn:
        from ..loader.device_dataset import DeviceGraphDataset
        ds = DeviceGraphDataset(train_graphs, dev, B)
    else:
        ds = DeviceHeteroDataset(train_graphs, dev, B)
    opt_cls = OPTIM_DICT[optim_cfg.optim_type]
    kw = dict(lr=optim_cfg.lr, weight_decay=optim_cfg.weight_decay)
    flat = flat_optimizer and optim_cfg.optim_type in ("adam", "adamW")   # optim.FlatAdam: the update as ONE launch
    if flat:
        from ..optim import FlatAdam
        fkw = dict(kw, max_norm=CLIP_MAX_NORM if clip else None, zero_grads=acc)    # clip + zeroing: in its launch
        optimizer = lambda st: FlatAdam.from_config(optim_cfg.optim_type, st.param_grads, st.grads, **fkw)  # noqa: E731
        capturable = True
    else:
        try:
            optimizer = opt_cls(model.parameters(), capturable=True, fused=True, **kw)
        except (TypeError, RuntimeError):          # (Adagrad has neither switch: its step stays outside the graph)
            optimizer = opt_cls(model.parameters(), **kw)
        capturable = bool(optimizer.defaults.get("capturable", False))
    in_graph = capturable      # the whole iteration -- backward, gradient all-reduce (if any), optimizer step -- is one graph
    gen = torch.Generator(device=dev).manual_seed(seed)
    model.train()
    model.engine = "resident"
    ds.new_epoch(gen)
    # the gather of the next permutation slice is captured in front of the step: a replay = next batch + iteration
    step = CapturedStep(model, ds.static, training_cfg.loss_fn, optimizer=optimizer if in_graph else None,
                        pre=ds.gather_next, reducer=reducer if in_graph else None, accumulate=acc,
                        max_norm=CLIP_MAX_NORM if clip and in_graph and not flat else None)
    if flat:
        optimizer = step.optimizer
    flat_grads = step.step.grads[:step.step.P]         # every parameter gradient (the loss column excluded)
    clip_norm = torch.zeros(1, dtype=torch.float32, device=dev) if clip and not in_graph else None

    def boundary_outside_graph(weight: float):
        """What the graph does not hold at a stepping iteration (a non-capturable optimizer; the eager tail)."""
        if reducer is not None:
            reducer.reduce(weight, weight * reducer.world_size)
        if flat:
            optimizer.step()                   # (clip and zeroing in the same launch)
            return
        if clip:
            clip_grad_norm_flat(flat_grads, CLIP_MAX_NORM, clip_norm if clip_norm is not None else step.clip_norm)
        optimizer.step()
        if acc:
            flat_grads.zero_()

    steps, tail = G // B, G % B
    num_batches = steps + (1 if tail else 0)
    legacy = not acc and not clip              # (the iteration exactly as before either setting existed)
    C = ds.C
    loss_log = torch.zeros(steps + (1 if tail else 0), dtype=torch.float32, device=dev)
    want_metric = metric_fn is not None or metric is not None
    scores = torch.zeros(G, C, dtype=torch.float32, device=dev) if want_metric else None
    targets = torch.zeros(G, C, dtype=torch.float32, device=dev) if want_metric else None
    eval_metric_fn = metric_fn
    if metric is not None:
        from .. import metrics as _metrics
        train_metric = _metrics.metric_buffers(metric, G, C, dev)
        train_loss = train_metric.packed[20:24].view(torch.float32)     # beside result and flags: one read-back
        launch = _metrics.average_precision_launch if metric == "ap" else _metrics.mean_absolute_error_launch
        eval_metric_fn = _metrics.eval_ap_hip if metric == "ap" else _metrics.eval_mae_hip    # (host loaders)
    evaluators = None
    if eval_graphs is not None:
        from .eval_resident import DeviceEvaluator
        evaluators = [DeviceEvaluator(g, model, training_cfg.loss_fn, B, metric) for g in eval_graphs]
    history, best, stale = [], float("inf"), 0
    for epoch in range(training_cfg.epochs):
        start = time.time()
        model.train()
        perm = ds.new_epoch(gen)               # permutation + batch counter on the device
        if epoch_orders is not None:
            epoch_orders.append(perm.cpu())
        if not in_graph:
            step.bind_grads()                  # (the eager tail of the previous epoch re-pointed p.grad)
        for i in range(steps):
            if legacy:
                step.replay()
                if reducer is not None and not in_graph:
                    reducer.reduce(float(B), float(B * reducer.world_size))
                if not in_graph:
                    optimizer.step()
            else:
                stepping = optimizer_steps_at(i, num_batches, k)
                step.replay(step_optimizer=stepping)
                if stepping and not in_graph:
                    boundary_outside_graph(float(B))
            loss_log[i].copy_(step.loss)
            if want_metric:
                scores[i * B:(i + 1) * B].copy_(step.score)
                targets[i * B:(i + 1) * B].copy_(ds.static.batch.y if mpnn else ds.static.batch["local"].y)
        if tail:
            tail_graphs = [train_graphs[j] for j in perm[steps * B:].tolist()]
            if mpnn:                           # (the layered engine: gradients are on)
                hb = Batch.from_data_list(tail_graphs).to(dev)
                hb.x = hb.x.float()
                optimizer.zero_grad(set_to_none=True)
                pred = model(hb)
                tail_y = hb.y
            else:
                hb = HeteroBatch.from_data_list(tail_graphs).to(dev)
                optimizer.zero_grad(set_to_none=True)
                pred = model(hb.x_dict, hb.edge_index_dict, hb)
                tail_y = hb["local"].y
            loss, score = criterion(training_cfg.loss_fn, pred, tail_y)
            loss.backward()
            if legacy:
                if reducer is not None:
                    reducer.reduce(float(tail), float(tail * reducer.world_size))
                optimizer.step_from_autograd() if flat else optimizer.step()
            elif flat and reducer is None:
                optimizer.step_from_autograd(accumulate=acc)     # (p.grad added to the window's sum; clip, zero)
            else:
                # the last batch steps (optimizer_steps_at); the window's earlier micro-batches are in the flat
                # buffer: the tail's p.grad is added to them there, and p.grad points at the sum again
                with torch.no_grad():
                    for p, g in step.grads:
                        if p.grad is None:
                            if not acc:
                                g.zero_()
                        elif p.grad.data_ptr() != g.data_ptr():
                            g.add_(p.grad) if acc else g.copy_(p.grad)
                step.bind_grads()
                boundary_outside_graph(float(tail))
            loss_log[steps].copy_(loss.detach())
            if want_metric:
                scores[steps * B:].copy_(score.detach())
                targets[steps * B:].copy_(tail_y)
            del pred, loss, score, hb
        if metric is not None:
            launch(targets, scores, out=train_metric)
            train_loss.copy_(loss_log.mean())
            f64, i32 = _metrics.read_packed(train_metric.packed)      # the epoch's only read-back
            mean_loss = float(i32[1:2].view(torch.float32)[0])
            perf = _metrics.metric_value(metric, float(f64[0]), int(i32[0]))
        else:
            mean_loss = float(loss_log.mean().item())                 # the epoch's only read-back
            perf = metric_fn(targets, scores) if metric_fn else float("nan")
        history.append((mean_loss, perf))
        if logger is not None:
            logger.info(f"epoch {epoch} train loss {mean_loss:.5f} perf {perf:.5f} ({time.time() - start:.2f}s)")
        if is_eval_epoch(epoch, training_cfg.epochs, training_cfg.eval_period):
            sources = evaluators if evaluators is not None else eval_loaders or []
            for split, source in zip(["Validation", "Test"], sources):
                if evaluators is not None:
                    vloss, vperf = source.evaluate()
                    if metric_fn is not None:
                        vperf = metric_fn(source.targets, source.scores)
                    if logger is not None:
                        logger.info(f"epoch {epoch} {split} loss {vloss:.5f} perf {vperf:.5f}")
                else:
                    vloss, vperf = eval_epoch(epoch, logger, source, model, training_cfg.loss_fn, eval_metric_fn, split)
                if eval_history is not None:
                    eval_history.append((epoch, split, vloss, vperf))
                if split == "Validation":
                    if reducer is not None and reducer.world_size > 1:
                        # every rank must take the same stop decision (the next collective would hang otherwise):
                        # the ranks agree on the mean of their validation losses
                        import torch.distributed as dist
                        t = torch.tensor([vloss], dtype=torch.float64, device=dev)
                        dist.all_reduce(t, group=reducer.group)
                        vloss = float(t.item()) / reducer.world_size
                    if vloss < best - training_cfg.min_delta:
                        best, stale = vloss, 0
                    else:
                        stale += 1
                    if stale >= training_cfg.patience and epoch != training_cfg.epochs - 1:
                        if logger is not None:
                            logger.info("stopping early")
                        ds.check()
                        return history
    ds.check()
    return history
