"""SAN's layer in GraphGPS's form (``SANLayer``): the attention over real and fake edges, then a feed-forward block,
each behind dropout, a residual connection and a normalisation:

    h = norm(x + O_h(drop(attention(x, edge_index, edge_attr))))
    h = norm(h + Linear(2D -> D)(drop(relu(Linear(D -> 2D)(h)))))

``attention`` is ``nn.attention.SANAttention`` (csrc/san.hip); ``O_h`` is a Linear with bias; the norms are the
package's own (``nn.norm``: "layer", "batch" or None).  The edge features pass through unchanged: every layer reads the
model's encoded ``edge_attr`` and the model's one fake-edge row."""
from __future__ import annotations

from typing import Optional

import torch.nn as nn
from torch import Tensor

from . import functional as Fh
from .attention import SANAttention
from .conv import Linear
from .gps import NORMS, _norm


class SANLayer(nn.Module):
    def __init__(self, channels: int, num_heads: int, gamma: float = 1e-1, full_graph: bool = True,
                 dropout: float = 0.0, norm: Optional[str] = "layer", attn_dropout: float = 0.0,
                 gamma_learn: bool = False):
        super().__init__()
        if norm not in NORMS:
            raise ValueError(f"norm must be 'layer', 'batch' or None, got {norm!r}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.channels, self.dropout = int(channels), float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks; None = nn.functional.dropout's default
        self.attention = SANAttention(channels, num_heads, gamma, full_graph, attn_dropout, gamma_learn)
        self.O_h = Linear(channels, channels)
        self.norm1_h = _norm(norm, channels)
        self.FFN_h_layer1 = Linear(channels, 2 * channels)
        self.FFN_h_layer2 = Linear(2 * channels, channels)
        self.norm2_h = _norm(norm, channels)

    @property
    def full_graph(self) -> bool:
        return self.attention.full_graph

    def _drop(self, x: Tensor, k: int) -> Tensor:
        seed = None if self.dropout_seed is None else self.dropout_seed + k
        return Fh.dropout(x, p=self.dropout, training=self.training, seed=seed)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Tensor, batch=None,
                fake_edge_row: Optional[Tensor] = None, *, ptr32: Optional[Tensor] = None,
                max_nodes: Optional[int] = None) -> Tensor:
        """``edge_attr``: [E, channels], the encoded edge features; ``batch``: the ``Batch`` (graph boundaries), or
        ``ptr32`` and ``max_nodes``; ``fake_edge_row``: the model's ``fake_edge_emb.weight`` [1, channels] (read with
        ``full_graph`` only)."""
        h = self.attention(x, edge_index, edge_attr, batch, fake_edge_row, ptr32=ptr32, max_nodes=max_nodes)
        h = self._drop(h, 0)
        h = x + Fh.linear_wide(h, self.O_h.weight, self.O_h.bias)
        if self.norm1_h is not None:
            h = self.norm1_h(h)
        f = Fh.linear_wide(h, self.FFN_h_layer1.weight, self.FFN_h_layer1.bias, "relu")
        h = h + Fh.linear_wide(self._drop(f, 1), self.FFN_h_layer2.weight, self.FFN_h_layer2.bias)
        if self.norm2_h is not None:
            h = self.norm2_h(h)
        return h
