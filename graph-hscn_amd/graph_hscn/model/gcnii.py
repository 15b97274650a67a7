"""The GCNII model (extension; LRGB's "GCNII" rows): a node encoder (``Linear(F -> H)`` or "atom"), ``num_layers``
``nn.conv.GCN2Conv`` layers in LRGB's layer form

    x = x_0 = encode_nodes(batch)
    for l in 1 .. L:   x_in = x;  x = dropout(relu(GCN2Conv_l(x, x_0)));  x = x_in + x  if residual

-- every layer one launch over ONE self-loop ``Relation`` built once per forward, ``GCN2Conv_l`` built with ``layer=l``
so that its weight's share ``beta_l = log(theta / l + 1)`` decays with depth -- and ``GPS``'s head per task level
("graph": mean pool, two Linears; "node": the two Linears per node; "link": ``model/_common.py LinkLevel``).

``pos_enc`` (a ``config.LapPEConfig`` or ``config.RWSEConfig`` with ``dim_emb = hidden_channels``) puts the trainable
positional encoder of ``model/_common.py PosEnc`` beside the node encoder, which is then ``H - dim_pe`` wide.

The model takes a homogeneous ``Batch`` (its ``edge_attr``, if any, is not read) and offers the surface
``train.batching`` and ``train.train`` use for one.  It runs on the layered operators only."""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..config.config import ACT_DICT, GCNIIConfig
from ._common import POOL_MAX_WIDTH, LayeredModel  # noqa: F401  (POOL_MAX_WIDTH stays importable from here)
from ..nn import functional as Fh
from ..nn.conv import GCN2Conv
from ..structure import self_loop_relation_of

RESIDENT_REASON = ("GCNII's layers (model/gcnii.py GCNII): a GCN2Conv stack that reads the initial representation in "
                   "every layer has no one-launch, resident or captured form; the model runs on the layered operators")


class GCNII(LayeredModel):
    def __init__(self, num_features: int, hidden_channels: int, num_classes: int, num_layers: int,
                 activation: Optional[Callable] = None, dropout: float = 0.0, alpha: float = 0.1,
                 theta: Optional[float] = 0.5, shared_weights: bool = True, residual: bool = False,
                 task_level: str = "graph", node_encoder: Optional[str] = None, pos_enc=None,
                 pe_undirected: bool = True) -> None:
        """``activation``: the head's (the layers' is ReLU, as LRGB's GCN2ConvLayer has it)."""
        super().__init__()
        self._check_args(node_encoder, None, task_level, num_layers)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        # (pinned masks: layer l = 1 .. L draws with dropout_seed + l)
        self._record(task_level, num_layers, activation, dropout, node_encoder, None)
        self.residual = bool(residual)
        H = int(hidden_channels)
        self._build_node_encoder(num_features, H, pos_enc, pe_undirected)
        self.layers = nn.ModuleList(GCN2Conv(H, alpha, theta, l, shared_weights) for l in range(1, num_layers + 1))
        self._build_head(H, num_classes)
        self._build_pos_encoder(H)                  # after every parameter of before

    def _own_reason(self) -> str:                   # (the GCN2Conv launches have no flag word: no _check_launch_flags)
        return RESIDENT_REASON

    # ---- forward -----------------------------------------------------------------------------------------------
    def _nodes(self, batch) -> Tensor:
        """[N, H] after the last layer."""
        x = x0 = self.encode_nodes(batch)
        rel = self_loop_relation_of(batch.edge_index, x.size(0), both=torch.is_grad_enabled())   # ONE for all layers
        for l, conv in enumerate(self.layers, start=1):
            x_in = x
            x = conv(x, x0, rel, act="relu")
            x = Fh.dropout(x, p=self.dropout, training=self.training,
                           seed=None if self.dropout_seed is None else self.dropout_seed + l)
            if self.residual:
                x = x_in + x
        return x


def build_gcnii(model_cfg: GCNIIConfig, num_features: int, num_classes: int) -> GCNII:
    return GCNII(num_features, model_cfg.hidden_channels, num_classes, model_cfg.num_layers,
                 ACT_DICT[model_cfg.activation.lower()], model_cfg.dropout, model_cfg.alpha, model_cfg.theta,
                 model_cfg.shared_weights, model_cfg.residual, model_cfg.task_level, model_cfg.node_encoder,
                 model_cfg.pos_enc, model_cfg.pe_undirected)
