"""GraphGPS's layer (Rampasek et al., "Recipe for a General, Powerful, Scalable Graph Transformer", 2022): a local
message-passing convolution and global self-attention side by side, then a feed-forward block, each behind a residual
connection, dropout and a normalisation:

    h_l = norm(x + drop(conv(x, edge_index[, edge_attr])))
    h_a = norm(x + drop(attn(x)))
    h   = h_l + h_a
    h   = norm(h + drop(Linear(2D -> D)(drop(act(Linear(D -> 2D)(h))))))

``local_conv="gatedgcn"`` is GraphGPS's published pairing: the local branch is a ``GatedGCNLayer``, which does its own
normalisation, activation, dropout and residual, so the layer adds no second dropout or residual around it
(``h_l = norm(GatedGCNLayer(x, e))``), and it updates the edge features: such a layer returns ``(h, edge_attr_out)``
and the model hands the second to the next layer.  Every other layer returns a Tensor.

``global_model="exphormer"`` puts ``ExphormerAttention`` -- sparse attention over the batch's own edges, an expander and
virtual nodes -- where ``MultiheadSelfAttention`` stands; the virtual rows travel beside ``x`` (``forward(exph=...)``).

``local_conv=None`` leaves the local branch out (``h = h_a``): the plain Transformer layer of the LRGB
"Transformer + PE" baselines.  Every operator is the package's own HIP one: the registry's convolutions,
``MultiheadSelfAttention``, ``Linear`` with the activation in its epilogue, the counter-based dropout and the norms."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from .._hip import ACT
from . import functional as Fh
from .attention import ExphormerAttention, MultiheadSelfAttention
from .conv import GatedGCNLayer, Linear
from .norm import BatchNorm1d, LayerNorm

LOCAL_CONVS = ("gcn", "gat", "gine", "gatedgcn", "transformerconv", "transformerconv_edge", "pna", "pna_edge")
NORMS = ("layer", "batch", None)
GLOBAL_MODELS = ("attention", "exphormer")


def _norm(kind: Optional[str], channels: int) -> Optional[nn.Module]:
    if kind == "layer":
        return LayerNorm(channels)
    if kind == "batch":
        return BatchNorm1d(channels)
    return None


class GPSLayer(nn.Module):
    def __init__(self, channels: int, local_conv: Optional[str], num_heads: int, dropout: float = 0.0,
                 norm: Optional[str] = "layer", act: str = "relu", spd_buckets: Optional[int] = None,
                 global_model: str = "attention", num_virtual_nodes: int = 0, pna=None):
        super().__init__()
        if global_model not in GLOBAL_MODELS:
            raise ValueError(f"global_model must be one of {GLOBAL_MODELS}, got {global_model!r}")
        if global_model == "exphormer" and spd_buckets is not None:
            raise ValueError("global_model='exphormer' has no shortest-path bias (spd_buckets must be None)")
        self.global_model = global_model
        from ..config.config import CONV_DICT, pna_kwargs
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
        if pna is not None and local_conv not in ("pna", "pna_edge"):
            raise ValueError(f"pna=PNAConfig(...) needs local_conv 'pna' or 'pna_edge', got {local_conv!r}")
        self.channels, self.local_conv, self.act, self.dropout = int(channels), local_conv, act, float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks; None = nn.functional.dropout's default
        if local_conv == "gatedgcn":        # GraphGPS's layer: batch norm, activation, dropout and residual inside
            self.conv = GatedGCNLayer(channels, dropout, residual=True, act=act)
        elif local_conv in ("transformerconv", "transformerconv_edge"):     # num_heads heads of width channels / num_heads
            if channels % num_heads:
                raise ValueError(f"channels {channels} must be divisible by num_heads {num_heads}")
            self.conv = CONV_DICT[local_conv](channels, channels // num_heads, heads=num_heads)
        elif local_conv in ("pna", "pna_edge"):     # pna: a config.PNAConfig (aggregators, scalers, avg_deg_log) or None
            self.conv = CONV_DICT[local_conv](channels, channels, **pna_kwargs(pna))
        else:
            self.conv = CONV_DICT[local_conv](channels, channels) if local_conv is not None else None
        # spd_buckets: the attention's own shortest-path bias table (Graphormer's spatial encoding); None: as before
        if global_model == "exphormer":     # sparse attention over the union graph in the dense attention's place
            self.attn = ExphormerAttention(channels, num_heads, num_virtual_nodes)
        else:
            self.attn = MultiheadSelfAttention(channels, num_heads, spd_buckets=spd_buckets)
        self.norm1_local = _norm(norm, channels) if local_conv is not None else None
        self.norm1_attn = _norm(norm, channels)
        self.ff_linear1 = Linear(channels, 2 * channels)
        self.ff_linear2 = Linear(2 * channels, channels)
        self.norm2 = _norm(norm, channels)

    @property
    def uses_edge_attr(self) -> bool:
        return bool(getattr(self.conv, "uses_edge_attr", False))

    @property
    def updates_edge_attr(self) -> bool:
        return bool(getattr(self.conv, "updates_edge_attr", False))

    def _drop(self, x: Tensor, k: int) -> Tensor:
        seed = None if self.dropout_seed is None else self.dropout_seed + k
        return Fh.dropout(x, p=self.dropout, training=self.training, seed=seed)

    def forward(self, x: Tensor, edge_index, batch=None, edge_attr: Optional[Tensor] = None, *,
                ptr32: Optional[Tensor] = None, max_nodes: Optional[int] = None, spd=None, exph=None):
        """``batch``: the ``Batch`` (graph boundaries of the attention), or ``ptr32`` and ``max_nodes``.  ``spd``: the
        batch's ``SPDBuckets``, for a layer built with ``spd_buckets`` (refused by name otherwise).  ``edge_attr``
        is read by an edge-aware ``local_conv`` ("gine", "gatedgcn", "transformerconv_edge", "pna_edge") only.  Returns the node features; with a
        ``local_conv`` that updates the edge features ("gatedgcn") the pair ``(h, edge_attr_out)``.

        ``global_model="exphormer"``: ``exph = (struct, virt, e_edge, e_type)`` -- the batch's ``ExphormerStructure``,
        the virtual rows [B nv, D] as the previous layer left them, the encoded local edge features (or None) and the
        edge-type embeddings.  The attention sees ``cat(x, virt)``; everything else of the layer runs on the node rows
        only, and the new virtual rows are appended to what the layer returns: ``(h, virt_out)`` or
        ``(h, edge_attr_out, virt_out)``."""
        edge_out = virt_out = None
        if self.global_model == "exphormer":
            if exph is None:
                raise ValueError("GPSLayer(global_model='exphormer') needs exph=(struct, virt, e_edge, e_type)")
            struct, virt, e_edge, e_type = exph
            h_a, virt_out = self.attn(torch.cat([x, virt], 0) if virt.size(0) else x, struct, e_edge, e_type)
        elif exph is not None:
            raise ValueError("exph= belongs to a layer built with global_model='exphormer'")
        else:                                       # (without buckets the call is that of before: no spd keyword)
            h_a = self.attn(x, batch, ptr32=ptr32, max_nodes=max_nodes, **({} if spd is None else {"spd": spd}))
        h_a = x + self._drop(h_a, 1)
        if self.norm1_attn is not None:
            h_a = self.norm1_attn(h_a)
        h = h_a
        if self.conv is not None:
            if self.uses_edge_attr:
                if edge_attr is None:
                    raise ValueError(f"local_conv {self.local_conv!r} needs edge_attr [E, De]")
            if self.updates_edge_attr:
                self.conv.dropout_seed = self.dropout_seed      # (+ 0: the seed the local branch's dropout has)
                h_l, edge_out = self.conv(x, edge_index, edge_attr)
            elif self.uses_edge_attr:
                h_l = x + self._drop(self.conv(x, edge_index, edge_attr), 0)
            else:
                h_l = x + self._drop(self.conv(x, edge_index), 0)
            if self.norm1_local is not None:
                h_l = self.norm1_local(h_l)
            h = h_l + h_a
        f = Fh.linear_wide(h, self.ff_linear1.weight, self.ff_linear1.bias, self.act)
        h = h + self._drop(Fh.linear_wide(self._drop(f, 2), self.ff_linear2.weight, self.ff_linear2.bias), 3)
        if self.norm2 is not None:
            h = self.norm2(h)
        if self.global_model == "exphormer":
            return (h, edge_out, virt_out) if self.updates_edge_attr else (h, virt_out)
        return (h, edge_out) if self.updates_edge_attr else h
