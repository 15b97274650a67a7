"""What the models spell alike, stated once: the validation of ``task_level`` (MPNN, GPS, HSCN) and of the categorical
encoders' names, the float ``edge_attr`` check and the link-level ``forward`` / ``embed`` pair of the two homogeneous
models (model/mpnn.py MPNN, model/gps.py GPS)."""
from __future__ import annotations

import torch
from torch import Tensor

from ..encoder.categorical import EDGE_ENCODERS, NODE_ENCODERS


def check_task_level(task_level) -> None:
    if task_level not in ("graph", "node", "link"):
        raise ValueError(f"task_level must be 'graph', 'node' or 'link', not {task_level!r}")


def check_encoders(node_encoder, edge_encoder) -> None:
    if node_encoder not in (None,) + tuple(NODE_ENCODERS):
        raise ValueError(f"node_encoder must be one of {sorted(NODE_ENCODERS)} or None, not {node_encoder!r}")
    if edge_encoder not in (None,) + tuple(EDGE_ENCODERS):
        raise ValueError(f"edge_encoder must be one of {sorted(EDGE_ENCODERS)} or None, not {edge_encoder!r}")


def float_edge_attr(ea: Tensor, dev) -> Tensor:
    """``batch.edge_attr`` of a model without an edge encoder: float32 on the model's device, or a TypeError."""
    if ea.dtype != torch.float32 or ea.device != dev:
        raise TypeError(f"edge_attr must be float32 on the model's device ({dev}); got {ea.dtype} on "
                        f"{ea.device} (train.batching.to_device casts integer bond features)")
    return ea


class LinkLevel:
    """Mixin of a homogeneous model with ``task_level`` and ``_forward(batch)``: at "link" level ``_forward`` gives the
    [N, D] node embeddings, ``forward`` scores the batch's candidate pairs with them and ``embed`` hands them out."""

    def forward(self, batch) -> Tensor:
        out = self._forward(batch)
        if self.task_level == "link":                  # one score per candidate pair of the batch
            from ..nn.head import PairStructure, pair_dot
            return pair_dot(out, batch.edge_label_index, PairStructure.of(batch, out.size(0)))
        return out

    def embed(self, batch) -> Tensor:
        """The [N, D] node embeddings a link-level model scores pairs with: the node-level model's forward."""
        if self.task_level != "link":
            raise RuntimeError("embed() belongs to a link-level model (task_level='link')")
        return self._forward(batch)
