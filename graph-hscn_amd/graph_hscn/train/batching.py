"""The one place that knows stage C's two batch kinds: ``HSCN`` takes a ``HeteroBatch`` (targets on the local node
type); every other model -- the MPNN baseline -- a homogeneous ``Batch`` with float32 features (the reference casts
them in its loop, train/train.py:79).  The eager loop, the captured loop, the device evaluator and
``replay.CapturedStep`` all ask here."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from ..data import Batch, HeteroBatch
from ..model.hscn import HSCN


def is_hetero(model) -> bool:
    return isinstance(model, HSCN)


def targets(model, batch) -> Optional[Tensor]:
    """The batch's targets, or ``None`` when it carries none."""
    if link_level(model):
        store = batch["local"] if is_hetero(model) else batch
        return store.edge_label if "edge_label" in store else None
    if is_hetero(model):
        return batch["local"].y if "y" in batch["local"] else None
    return getattr(batch, "y", None)


def class_index_targets(y: Optional[Tensor]) -> bool:
    """Whether ``y`` holds one class index per graph (the criterion's multiclass branch) rather than ``[B, C]``."""
    return y is not None and y.dim() == 1 and not y.dtype.is_floating_point


def score_width(model, y: Tensor) -> int:
    """Columns of the score ``criterion`` returns for targets ``y``: ``y``'s own for ``[B, C]`` targets; for class
    indices the width of the model's head (HSCN: ``lin_2``; a node-level MPNN: its last convolution)."""
    if not class_index_targets(y):
        return int(y.size(1))
    if not is_hetero(model) and hasattr(model, "head_width"):        # (model/gps.py GPS: no resident_dims)
        return int(model.head_width())
    if not is_hetero(model) and node_level(model):
        return int(model.resident_dims()[2])
    if not is_hetero(model):
        raise ValueError("class-index targets are served for HSCN (the reference model) only")
    return int(model.lin_2.out_channels)


def node_level(model) -> bool:
    return getattr(model, "task_level", "graph") == "node"


def refuse_node_level(model, what: str) -> None:
    """The one-launch and captured steps, ``fit_resident`` and ``DeviceEvaluator`` end in the per-graph pool: they
    refuse a node-level model by name, before anything is launched or captured -- they never pool silently."""
    if node_level(model):
        raise RuntimeError(f"{what} does not take this model: {model.resident_reason()} (train.train runs it)")


def refuse_layered_only(model, what: str) -> None:
    """The same for a model that has no resident form at all (``layered_only``: model/gps.py GPS, global attention)."""
    if getattr(model, "layered_only", False):
        raise RuntimeError(f"{what} does not take this model: {model.resident_reason()} (train.train runs it)")


def link_level(model) -> bool:
    return getattr(model, "task_level", "graph") == "link"


def refuse_link_level(model, what: str) -> None:
    """The same for a link-level model: those launches know neither candidate pairs nor a pair decoder."""
    if link_level(model):
        raise RuntimeError(f"{what} does not take this model: {model.resident_reason()} (train.train runs it)")


def link_forward(model, batch) -> Tuple[Tensor, Tensor, Tensor]:
    """``(scores, edge_label, z)`` of a link-level model: what ``forward`` answers plus the detached [N, D]
    embeddings the scores were taken from, which the epoch's ranking metric is fed with."""
    from ..nn.head import PairStructure, pair_dot
    if model.engine == "resident":
        refuse_link_level(model, "engine='resident'")
    if is_hetero(model):
        store, z = batch["local"], model.embed(batch.x_dict, batch.edge_index_dict, batch)
    else:
        store, z = batch, model.embed(batch)
    scores = pair_dot(z, store.edge_label_index, PairStructure.of(store, z.size(0)))
    return scores, store.edge_label, z.detach()


def forward(model, batch) -> Tuple[Tensor, Tensor]:
    """``(pred, targets)`` of ``model`` on a batch that is on the model's device.  A node-level model
    (``task_level="node"``) answers ``[N, C]`` and the targets are the per-node labels; a link-level model
    (``task_level="link"``) answers one score per candidate pair, ``[P]``, and the targets are ``edge_label``."""
    if node_level(model) and model.engine == "resident":
        refuse_node_level(model, "engine='resident'")
    if link_level(model):
        return link_forward(model, batch)[:2]
    if is_hetero(model):
        if getattr(model, "vl_conv", None) is not None and torch.is_grad_enabled() and model.engine == "resident":
            # the eager tail of a device loop: with gradients on this model runs through the layered operators
            model.engine = "auto"
            try:
                return model(batch.x_dict, batch.edge_index_dict, batch), batch["local"].y
            finally:
                model.engine = "resident"
        return model(batch.x_dict, batch.edge_index_dict, batch), batch["local"].y
    return model(batch), batch.y


def to_device(model, batch, device):
    """A loader's batch where the HIP operators can take it."""
    host = batch
    batch = batch.to(device)
    _carry_host_side(host, batch)
    if not is_hetero(model):
        # a categorical encoder (model.encoder_kinds: node, edge) reads its tensor as int64 categories
        node_enc, edge_enc = getattr(model, "encoder_kinds", (None, None))
        batch.x = batch.x.float() if node_enc is None else _categories(batch.x, "x")
        edge_attr = getattr(batch, "edge_attr", None)
        if edge_attr is not None:                   # OGB bond features are integers
            batch.edge_attr = edge_attr.float() if edge_enc is None else _categories(edge_attr, "edge_attr")
    return batch


def _carry_host_side(src, dst) -> None:
    """What a homogeneous batch keeps on the host beside its keys, handed from ``src`` to its copy ``dst``: every graph's
    node count (from ``ptr`` while that still lies on the host: integer work on the host, nothing read back) and the
    dict of what a model derives from the batch's structure once (model/gps.py: the shortest-path buckets, keyed by
    (max_dist, device)) -- ONE dict for the loader's batch and every copy made of it here, so a batch reused across
    epochs is computed once."""
    if not hasattr(src, "__dict__") or not hasattr(dst, "__dict__") or "ptr" not in getattr(src, "_d", {}):
        return
    sizes = src.__dict__.get("_host_sizes")
    if sizes is None and isinstance(src.ptr, Tensor) and not src.ptr.is_cuda:
        sizes = tuple(int(n) for n in (src.ptr[1:] - src.ptr[:-1]).tolist())
        src.__dict__["_host_sizes"] = sizes
    if sizes is not None:
        dst.__dict__["_host_sizes"] = sizes
    dst.__dict__["_spd_cache"] = src.__dict__.setdefault("_spd_cache", {})


def _categories(t: Tensor, name: str) -> Tensor:
    if t.is_floating_point():
        raise TypeError(f"the model has a categorical encoder for {name}, which reads integer categories; the batch "
                        f"carries {t.dtype}")
    return t.long()


def collate(model, graphs: Sequence, device):
    """Host collation of a graph list, onto ``device``."""
    return to_device(model, (HeteroBatch if is_hetero(model) else Batch).from_data_list(graphs), device)


def dataset_class(model):
    """``loader.device_dataset``'s class for the graphs ``model`` trains on."""
    from ..loader.device_dataset import DeviceGraphDataset, DeviceHeteroDataset
    return DeviceHeteroDataset if is_hetero(model) else DeviceGraphDataset


def resident_step(model, batch, loss_fn: str, one_launch: Optional[bool] = None, structure=None,
                  accumulate: bool = False):
    """The resident training step of ``model`` on a static batch (``step.ResidentTrainStep``; the MPNN baseline's or
    the vl model's one launch, which have neither a launch pair nor a structure to load)."""
    from ..step import MPNNResidentTrainStep, ResidentTrainStep, VLResidentTrainStep
    refuse_layered_only(model, "the resident training step")
    refuse_node_level(model, "the resident training step")
    refuse_link_level(model, "the resident training step")
    if targets(model, batch) is None:
        raise ValueError("the static batch carries no targets")
    if not is_hetero(model):
        return MPNNResidentTrainStep(model, batch, loss_fn, accumulate=accumulate)
    if getattr(model, "vl_conv", None) is not None:
        return VLResidentTrainStep(model, batch, loss_fn, accumulate=accumulate)
    try:
        return ResidentTrainStep(model, batch, loss_fn, one_launch=one_launch, structure=structure,
                                 accumulate=accumulate)
    except RuntimeError as e:
        raise RuntimeError("CapturedStep needs the graph-resident engine (the layered operators size their "
                           "work by tensor shapes, which a static-capacity batch does not carry): " + str(e)) from e
