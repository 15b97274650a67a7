"""The SAN model (extension; LRGB's "SAN + LapPE" / "SAN + RWSE" rows): a node encoder (``Linear(F -> D)`` or "atom"),
an edge encoder to width D (``Linear(-1, D)`` or "bond"), ``num_layers`` ``nn.san.SANLayer`` s -- attention over every
ordered pair of a graph, the listed edges through one set of projections and their features, all other pairs through
a second set and ONE learned fake-edge row ``fake_edge_emb.weight`` [1, D] that all layers share -- and ``GPS``'s head
per task level ("graph": mean pool, two Linears; "node": the two Linears per node; "link": ``model/_common.py
LinkLevel``).

``pos_enc`` (a ``config.LapPEConfig`` or ``config.RWSEConfig`` with ``dim_emb = hidden_channels``) puts the trainable
positional encoder of ``model/_common.py PosEnc`` beside the node encoder, which is then ``D - dim_pe`` wide.

The model takes a homogeneous ``Batch`` WITH ``edge_attr`` and offers the surface ``train.batching`` and ``train.train``
use for one.  It runs on the layered operators only: SAN's attention has no one-launch, resident or captured form."""
from __future__ import annotations

from typing import Callable, Optional

import torch.nn as nn
from torch import Tensor

from ..config.config import ACT_DICT, SANConfig
from ..encoder.categorical import EDGE_ENCODERS, NODE_ENCODERS, resident_reason as encoder_reason
from ._common import POSENC_RESIDENT_REASON, LinkLevel, PosEnc, check_encoders, check_task_level, float_edge_attr
from .gps import _Table
from ..nn import functional as Fh
from ..nn.conv import Linear
from ..nn.head import NodeHead
from ..nn.pool import global_mean_pool
from ..nn.san import SANLayer

RESIDENT_REASON = ("SAN's attention over real and fake edges (model/san.py SAN): full-graph attention with two kinds "
                   "of pairs has no one-launch, resident or captured form; the model runs on the layered operators")


class SAN(LinkLevel, PosEnc, nn.Module):
    layered_only = True      # train.batching.refuse_layered_only: the resident entry points refuse this model by name

    def __init__(self, num_features: int, hidden_channels: int, num_classes: int, num_layers: int, num_heads: int = 4,
                 activation: Optional[Callable] = None, dropout: float = 0.0, norm: Optional[str] = "layer",
                 task_level: str = "graph", node_encoder: Optional[str] = None, edge_encoder: Optional[str] = None,
                 gamma: float = 1e-1, full_graph: bool = True, pos_enc=None, pe_undirected: bool = True,
                 attn_dropout: float = 0.0, gamma_learn: bool = False) -> None:
        """``gamma`` >= 0: the fixed weight of the fake pairs against the real ones (a = 1 / (1 + gamma), b = gamma /
        (1 + gamma)); ``full_graph=False``: the listed edges alone (no second set of projections, no fake-edge row).
        ``gamma_learn`` and ``attn_dropout`` are refused by name.  ``activation``: the head's (the layers' feed-forward
        block is ReLU, as GraphGPS's ``SANLayer`` has it)."""
        super().__init__()
        check_encoders(node_encoder, edge_encoder)
        check_task_level(task_level)
        if num_layers < 1:
            raise ValueError("SAN needs at least one layer")
        activation = ACT_DICT["relu"] if activation is None else activation
        act = getattr(activation, "hscn_name", None)
        if act is None:
            raise ValueError("activation must be one of config.ACT_DICT's (it runs in a Linear's epilogue)")
        self.task_level = task_level
        self.num_layers = int(num_layers)
        self.activation = activation
        self.dropout = float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks (layer i draws with seeds + 2 i, + 2 i + 1)
        self.gamma, self.full_graph = Fh._check_gamma(gamma), bool(full_graph)
        D = int(hidden_channels)
        self.encoder_kinds = (node_encoder, edge_encoder)
        Dx = self._init_pos_enc(pos_enc, pe_undirected, D)             # D - dim_pe with a positional encoder
        self.node_encoder = Linear(num_features, Dx) if node_encoder is None else NODE_ENCODERS[node_encoder](Dx)
        self.edge_encoder = Linear(-1, D) if edge_encoder is None else EDGE_ENCODERS[edge_encoder](D)
        if self.full_graph:
            self.fake_edge_emb = _Table(1, D)
        self.layers = nn.ModuleList(SANLayer(D, num_heads, self.gamma, self.full_graph, dropout, norm, attn_dropout,
                                             gamma_learn) for _ in range(num_layers))
        self.lin_1 = Linear(D, D)
        self.lin_2 = Linear(D, num_classes)
        self._node_head = NodeHead(self.lin_1, self.lin_2, act)
        self._build_pos_encoder(D)                  # after every parameter of before
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
        """Synchronising: raises if a SAN attention launch since the last check skipped an edge that left its graph or
        met a graph larger than its batch's ``max_nodes`` (``nn.functional.check_san``); then the encoders' words, as
        ``GPS.check_flags`` reads them."""
        dev = next(self.parameters()).device
        Fh.check_san(dev)
        if any(self.encoder_kinds):                # the categorical encoders' (an index outside its column)
            Fh.check_categorical(dev)
        self._check_pe_flags()                      # and the positional encoder's statistics launches'

    # ---- forward -----------------------------------------------------------------------------------------------
    def _edge_attr(self, batch) -> Tensor:
        ea = getattr(batch, "edge_attr", None)
        if ea is None:
            raise ValueError("SAN's real pairs are scored through their edge features and the batch carries no "
                             "edge_attr (Data(edge_attr=[E, De]); make_dataset(..., edge_features=True))")
        if self.encoder_kinds[1] is not None:       # int64 categories: the bond encoder checks them itself
            return ea
        return float_edge_attr(ea, next(self.parameters()).device)

    def _embed_x(self, batch) -> Tensor:
        return self.node_encoder(batch.x)

    def _nodes(self, batch) -> Tensor:
        """[N, D] after the last SAN layer."""
        if self.engine not in ("layered", "auto", "resident"):
            raise ValueError(f"engine must be 'layered', 'auto' or 'resident', got {self.engine!r}")
        if self.engine == "resident":
            raise RuntimeError(f"engine='resident' does not take this model: {self.resident_reason()}")
        self.last_engine = "layered"
        edge_attr = self.edge_encoder(self._edge_attr(batch))
        x = self.encode_nodes(batch)
        fake = self.fake_edge_emb.weight if self.full_graph else None
        for i, layer in enumerate(self.layers):
            layer.dropout_seed = None if self.dropout_seed is None else self.dropout_seed + 2 * i
            x = layer(x, batch.edge_index, edge_attr, batch, fake)
        return x

    def _head(self, x: Tensor) -> Tensor:
        h = Fh.linear_wide(x, self.lin_1.weight, self.lin_1.bias, self.activation.hscn_name)
        return Fh.linear_wide(h, self.lin_2.weight, self.lin_2.bias)

    def _forward(self, batch) -> Tensor:
        x = self._nodes(batch)
        if self.task_level == "graph":
            x = global_mean_pool(x, batch.batch, getattr(batch, "num_graphs", None))
            return self._head(x)
        return self._node_head(x) if self._node_head.supported() else self._head(x)


def build_san(model_cfg: SANConfig, num_features: int, num_classes: int) -> SAN:
    return SAN(num_features, model_cfg.hidden_channels, num_classes, model_cfg.num_layers, model_cfg.num_heads,
               ACT_DICT[model_cfg.activation.lower()], model_cfg.dropout, model_cfg.norm, model_cfg.task_level,
               model_cfg.node_encoder, model_cfg.edge_encoder, model_cfg.gamma, model_cfg.full_graph,
               model_cfg.pos_enc, model_cfg.pe_undirected)
