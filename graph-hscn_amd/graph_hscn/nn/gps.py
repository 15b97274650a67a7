"""GraphGPS's layer (Rampasek et al., "Recipe for a General, Powerful, Scalable Graph Transformer", 2022): a local
message-passing convolution and global self-attention side by side, then a feed-forward block, each behind a residual
connection, dropout and a normalisation:

    h_l = norm(x + drop(conv(x, edge_index[, edge_attr])))
    h_a = norm(x + drop(attn(x)))
    h   = h_l + h_a
    h   = norm(h + drop(Linear(2D -> D)(drop(act(Linear(D -> 2D)(h))))))

``local_conv=None`` leaves the local branch out (``h = h_a``): the plain Transformer layer of the LRGB
"Transformer + PE" baselines.  Every operator is the package's own HIP one: the registry's convolutions,
``MultiheadSelfAttention``, ``Linear`` with the activation in its epilogue, the counter-based dropout and the norms."""
from __future__ import annotations

from typing import Optional

import torch.nn as nn
from torch import Tensor

from .._hip import ACT
from . import functional as Fh
from .attention import MultiheadSelfAttention
from .conv import Linear
from .norm import BatchNorm1d, LayerNorm

LOCAL_CONVS = ("gcn", "gat", "gine")
NORMS = ("layer", "batch", None)


def _norm(kind: Optional[str], channels: int) -> Optional[nn.Module]:
    if kind == "layer":
        return LayerNorm(channels)
    if kind == "batch":
        return BatchNorm1d(channels)
    return None


class GPSLayer(nn.Module):
    def __init__(self, channels: int, local_conv: Optional[str], num_heads: int, dropout: float = 0.0,
                 norm: Optional[str] = "layer", act: str = "relu"):
        super().__init__()
        from ..config.config import CONV_DICT
        if local_conv is not None:
            local_conv = local_conv.lower()
            if local_conv not in LOCAL_CONVS:
                raise ValueError(f"local_conv must be one of {LOCAL_CONVS} or None, got {local_conv!r}")
        if norm not in NORMS:
            raise ValueError(f"norm must be 'layer', 'batch' or None, got {norm!r}")
        if act not in ACT:
            raise ValueError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.channels, self.local_conv, self.act, self.dropout = int(channels), local_conv, act, float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks; None = nn.functional.dropout's default
        self.conv = CONV_DICT[local_conv](channels, channels) if local_conv is not None else None
        self.attn = MultiheadSelfAttention(channels, num_heads)
        self.norm1_local = _norm(norm, channels) if local_conv is not None else None
        self.norm1_attn = _norm(norm, channels)
        self.ff_linear1 = Linear(channels, 2 * channels)
        self.ff_linear2 = Linear(2 * channels, channels)
        self.norm2 = _norm(norm, channels)

    @property
    def uses_edge_attr(self) -> bool:
        return bool(getattr(self.conv, "uses_edge_attr", False))

    def _drop(self, x: Tensor, k: int) -> Tensor:
        seed = None if self.dropout_seed is None else self.dropout_seed + k
        return Fh.dropout(x, p=self.dropout, training=self.training, seed=seed)

    def forward(self, x: Tensor, edge_index, batch=None, edge_attr: Optional[Tensor] = None, *,
                ptr32: Optional[Tensor] = None, max_nodes: Optional[int] = None) -> Tensor:
        """``batch``: the ``Batch`` (graph boundaries of the attention), or ``ptr32`` and ``max_nodes``.  ``edge_attr``
        is read by an edge-aware ``local_conv`` ("gine") only."""
        h_a = self.attn(x, batch, ptr32=ptr32, max_nodes=max_nodes)
        h_a = x + self._drop(h_a, 1)
        if self.norm1_attn is not None:
            h_a = self.norm1_attn(h_a)
        h = h_a
        if self.conv is not None:
            if self.uses_edge_attr:
                if edge_attr is None:
                    raise ValueError("local_conv 'gine' needs edge_attr [E, De]")
                h_l = self.conv(x, edge_index, edge_attr)
            else:
                h_l = self.conv(x, edge_index)
            h_l = x + self._drop(h_l, 0)
            if self.norm1_local is not None:
                h_l = self.norm1_local(h_l)
            h = h_l + h_a
        f = Fh.linear_wide(h, self.ff_linear1.weight, self.ff_linear1.bias, self.act)
        h = h + self._drop(Fh.linear_wide(self._drop(f, 2), self.ff_linear2.weight, self.ff_linear2.bias), 3)
        if self.norm2 is not None:
            h = self.norm2(h)
        return h
