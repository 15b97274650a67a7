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
from ..encoder.categorical import EDGE_ENCODERS
from ._common import LayeredModel, _Table
from ..nn import functional as Fh
from ..nn.conv import Linear
from ..nn.san import SANLayer

RESIDENT_REASON = ("SAN's attention over real and fake edges (model/san.py SAN): full-graph attention with two kinds "
                   "of pairs has no one-launch, resident or captured form; the model runs on the layered operators")


class SAN(LayeredModel):
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
        self._check_args(node_encoder, edge_encoder, task_level, num_layers)
        # (pinned masks: layer i draws with dropout_seed + 2 i, + 2 i + 1)
        self._record(task_level, num_layers, activation, dropout, node_encoder, edge_encoder)
        self.gamma, self.full_graph = Fh._check_gamma(gamma), bool(full_graph)
        D = int(hidden_channels)
        self._build_node_encoder(num_features, D, pos_enc, pe_undirected)
        self.edge_encoder = Linear(-1, D) if edge_encoder is None else EDGE_ENCODERS[edge_encoder](D)
        if self.full_graph:
            self.fake_edge_emb = _Table(1, D)
        self.layers = nn.ModuleList(SANLayer(D, num_heads, self.gamma, self.full_graph, dropout, norm, attn_dropout,
                                             gamma_learn) for _ in range(num_layers))
        self._build_head(D, num_classes)
        self._build_pos_encoder(D)                  # after every parameter of before

    # ---- what LayeredModel asks of the model ---------------------------------------------------------------------
    def _own_reason(self) -> str:
        return RESIDENT_REASON

    def _check_launch_flags(self, dev) -> None:
        """A SAN attention launch that skipped an edge that left its graph or met a graph larger than its batch's
        ``max_nodes``."""
        Fh.check_san(dev)

    def _edge_attr_reader(self) -> str:
        return "SAN's real pairs are scored through their edge features"

    # ---- forward -----------------------------------------------------------------------------------------------
    def _nodes(self, batch) -> Tensor:
        """[N, D] after the last SAN layer."""
        edge_attr = self.edge_encoder(self._edge_attr(batch))
        x = self.encode_nodes(batch)
        fake = self.fake_edge_emb.weight if self.full_graph else None
        for i, layer in enumerate(self.layers):
            layer.dropout_seed = None if self.dropout_seed is None else self.dropout_seed + 2 * i
            x = layer(x, batch.edge_index, edge_attr, batch, fake)
        return x


def build_san(model_cfg: SANConfig, num_features: int, num_classes: int) -> SAN:
    return SAN(num_features, model_cfg.hidden_channels, num_classes, model_cfg.num_layers, model_cfg.num_heads,
               ACT_DICT[model_cfg.activation.lower()], model_cfg.dropout, model_cfg.norm, model_cfg.task_level,
               model_cfg.node_encoder, model_cfg.edge_encoder, model_cfg.gamma, model_cfg.full_graph,
               model_cfg.pos_enc, model_cfg.pe_undirected)
