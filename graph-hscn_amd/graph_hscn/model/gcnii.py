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
from ..encoder.categorical import NODE_ENCODERS, resident_reason as encoder_reason
from ._common import POSENC_RESIDENT_REASON, LinkLevel, PosEnc, check_encoders, check_task_level
from ..nn import functional as Fh
from ..nn.conv import GCN2Conv, Linear
from ..nn.head import NodeHead
from ..nn.pool import global_mean_pool
from ..structure import self_loop_relation_of

# hscn_segment_mean_fwd (csrc/pool.hip) gives a row at most 64 lanes of four columns
POOL_MAX_WIDTH = 256
RESIDENT_REASON = ("GCNII's layers (model/gcnii.py GCNII): a GCN2Conv stack that reads the initial representation in "
                   "every layer has no one-launch, resident or captured form; the model runs on the layered operators")


class GCNII(LinkLevel, PosEnc, nn.Module):
    layered_only = True      # train.batching.refuse_layered_only: the resident entry points refuse this model by name

    def __init__(self, num_features: int, hidden_channels: int, num_classes: int, num_layers: int,
                 activation: Optional[Callable] = None, dropout: float = 0.0, alpha: float = 0.1,
                 theta: Optional[float] = 0.5, shared_weights: bool = True, residual: bool = False,
                 task_level: str = "graph", node_encoder: Optional[str] = None, pos_enc=None,
                 pe_undirected: bool = True) -> None:
        """``activation``: the head's (the layers' is ReLU, as LRGB's GCN2ConvLayer has it)."""
        super().__init__()
        check_encoders(node_encoder, None)
        check_task_level(task_level)
        if num_layers < 1:
            raise ValueError("GCNII needs at least one layer")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        activation = ACT_DICT["relu"] if activation is None else activation
        act = getattr(activation, "hscn_name", None)
        if act is None:
            raise ValueError("activation must be one of config.ACT_DICT's (it runs in a Linear's epilogue)")
        self.task_level = task_level
        self.num_layers = int(num_layers)
        self.activation = activation
        self.dropout = float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks (layer l = 1 .. L draws with seed + l)
        self.residual = bool(residual)
        H = int(hidden_channels)
        self.encoder_kinds = (node_encoder, None)
        Hx = self._init_pos_enc(pos_enc, pe_undirected, H)             # H - dim_pe with a positional encoder
        self.node_encoder = Linear(num_features, Hx) if node_encoder is None else NODE_ENCODERS[node_encoder](Hx)
        self.layers = nn.ModuleList(GCN2Conv(H, alpha, theta, l, shared_weights) for l in range(1, num_layers + 1))
        self.lin_1 = Linear(H, H)
        self.lin_2 = Linear(H, num_classes)
        self._node_head = NodeHead(self.lin_1, self.lin_2, act)
        self._build_pos_encoder(H)                  # after every parameter of before
        # "layered"; "auto" runs layered too; "resident" raises with the reason when the model is called
        self.engine = "layered"
        self.last_engine: Optional[str] = None

    # ---- the surface of a homogeneous model (train.batching, train.train) ----------------------------------------
    def resident_reason(self, batch=None, need_grad: bool = False) -> str:
        reason = RESIDENT_REASON
        if self.pos_enc is not None:
            reason = reason + "; " + POSENC_RESIDENT_REASON
        if any(self.encoder_kinds):
            return reason + "; " + encoder_reason(*self.encoder_kinds)
        return reason

    def supported(self, batch=None) -> bool:
        return False

    def head_width(self) -> int:
        """Columns of the prediction (what ``batching.score_width`` asks for class-index targets)."""
        return int(self.lin_2.out_channels)

    def check_flags(self) -> None:
        """Synchronising: raises for a flag word of the categorical encoder (an index outside its column) or of the
        positional encoder's statistics launches; the GCN2Conv launches have none."""
        if any(self.encoder_kinds):
            Fh.check_categorical(next(self.parameters()).device)
        self._check_pe_flags()

    # ---- forward -----------------------------------------------------------------------------------------------
    def _embed_x(self, batch) -> Tensor:
        return self.node_encoder(batch.x)

    def _nodes(self, batch) -> Tensor:
        """[N, H] after the last layer."""
        if self.engine not in ("layered", "auto", "resident"):
            raise ValueError(f"engine must be 'layered', 'auto' or 'resident', got {self.engine!r}")
        if self.engine == "resident":
            raise RuntimeError(f"engine='resident' does not take this model: {self.resident_reason()}")
        self.last_engine = "layered"
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

    def _pool(self, x: Tensor, batch) -> Tensor:
        """[B, H] graph means.  The mean pool's kernel takes ``POOL_MAX_WIDTH`` columns: a wider x (H = 300, the LRGB
        width) is pooled in column slices of that many, a column's mean being the same sum either way."""
        num_graphs = getattr(batch, "num_graphs", None)
        if x.size(1) <= POOL_MAX_WIDTH:
            return global_mean_pool(x, batch.batch, num_graphs)
        parts = [global_mean_pool(x[:, c:c + POOL_MAX_WIDTH].contiguous(), batch.batch, num_graphs)
                 for c in range(0, x.size(1), POOL_MAX_WIDTH)]
        return torch.cat(parts, 1)

    def _head(self, x: Tensor) -> Tensor:
        h = Fh.linear_wide(x, self.lin_1.weight, self.lin_1.bias, self.activation.hscn_name)
        return Fh.linear_wide(h, self.lin_2.weight, self.lin_2.bias)

    def _forward(self, batch) -> Tensor:
        x = self._nodes(batch)
        if self.task_level == "graph":
            return self._head(self._pool(x, batch))
        return self._node_head(x) if self._node_head.supported() else self._head(x)


def build_gcnii(model_cfg: GCNIIConfig, num_features: int, num_classes: int) -> GCNII:
    return GCNII(num_features, model_cfg.hidden_channels, num_classes, model_cfg.num_layers,
                 ACT_DICT[model_cfg.activation.lower()], model_cfg.dropout, model_cfg.alpha, model_cfg.theta,
                 model_cfg.shared_weights, model_cfg.residual, model_cfg.task_level, model_cfg.node_encoder,
                 model_cfg.pos_enc, model_cfg.pe_undirected)
