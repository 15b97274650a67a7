"""Global attention: ``MultiheadSelfAttention`` is ``torch.nn.MultiheadAttention`` restricted to self-attention among
the nodes of each graph of a collated batch, on the HIP path (csrc/attention.hip): no padding, no mask tensor.

Parameters, their shapes, ``state_dict`` keys and the initialisation are torch's (``in_proj_weight`` [3D, D] xavier
uniform, ``in_proj_bias`` and ``out_proj.bias`` zero, ``out_proj.weight`` kaiming uniform with a = sqrt 5), so weights
move both ways with ``load_state_dict``.  Both projections run through the HIP ``linear`` (``linear_wide``: in column
chunks where the weight is wider than the kernel's LDS image); the attention itself is
``nn.functional.SelfAttentionFn``."""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as Fh


class _OutProj(nn.Module):
    """``out_proj`` of torch's module (a ``NonDynamicallyQuantizableLinear``): ``weight`` [D, D] and ``bias`` [D]."""

    def __init__(self, embed_dim: int, bias: bool):
        super().__init__()
        self.in_features = self.out_features = embed_dim
        self.weight = nn.Parameter(torch.empty(embed_dim, embed_dim))
        if bias:
            self.bias = nn.Parameter(torch.empty(embed_dim))
        else:
            self.register_parameter("bias", None)

    def forward(self, x: Tensor) -> Tensor:
        return Fh.linear_wide(x, self.weight, self.bias)


class _SPDBias(nn.Module):
    """Graphormer's spatial encoding: ``weight`` [num_buckets, num_heads], one learned scalar per (shortest-path bucket,
    head), added to the attention logit (an ``nn.Embedding``'s key, ``spd_bias.weight``)."""

    def __init__(self, num_buckets: int, num_heads: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_buckets, num_heads))


class MultiheadSelfAttention(nn.Module):
    """``forward(x, batch)``: x [N, D] float32 on the device, ``batch`` a ``graph_hscn.data.Batch`` (its ``ptr32`` and
    ``max_nodes`` say which rows form a graph) -> [N, D].  ``forward(x, ptr32=..., max_nodes=...)`` takes the two
    directly.

    ``spd_buckets=K`` adds Graphormer's spatial encoding: the module owns ``spd_bias.weight`` [K, num_heads] (drawn
    normal(0, 0.02) after every other parameter) and ``forward(x, batch, spd=...)`` takes the batch's ``SPDBuckets``
    (``nn.functional.shortest_path_buckets``) with ``max_dist + 1 == K``; logit (i, j) of head h gains
    ``spd_bias.weight[bucket_ij, h]`` (csrc/attention.hip).  Without it the module is what it always was.

    Not provided, refused by name: dropout on the attention weights, ``need_weights``, a dense attention bias tensor or
    any mask other than the graph boundary, ``spd=`` on a module without ``spd_buckets``, an ``embed_dim`` that
    ``num_heads`` does not divide, a head width outside the kernel's envelope, CPU tensors."""

    def __init__(self, embed_dim: int, num_heads: int, bias: bool = True, dropout: float = 0.0,
                 spd_buckets: Optional[int] = None):
        super().__init__()
        if spd_buckets is not None and not 2 <= int(spd_buckets) <= Fh.ATTN_MAX_BUCKETS:
            raise ValueError(f"MultiheadSelfAttention: spd_buckets must be max_dist + 1 with max_dist in "
                             f"[{Fh.SPD_MIN_DIST}, {Fh.SPD_MAX_DIST}], got {spd_buckets}")
        if embed_dim <= 0 or num_heads <= 0:
            raise ValueError(f"embed_dim and num_heads must be greater than 0, got embed_dim={embed_dim} and "
                             f"num_heads={num_heads} instead")
        if embed_dim % num_heads != 0:
            raise ValueError(f"embed_dim must be divisible by num_heads (got embed_dim={embed_dim}, "
                             f"num_heads={num_heads})")
        if dropout != 0.0:
            raise NotImplementedError("MultiheadSelfAttention(dropout > 0): dropout on the attention weights is not "
                                      "implemented (the weights never exist in memory); drop the layer's output instead")
        head_dim = embed_dim // num_heads
        if not (head_dim % 4 == 0 and Fh.ATTN_MIN_HEAD_DIM <= head_dim <= Fh.ATTN_MAX_HEAD_DIM
                and embed_dim <= Fh.ATTN_MAX_WIDTH):
            raise ValueError(f"MultiheadSelfAttention: embed_dim={embed_dim} with num_heads={num_heads} (head width "
                             f"{head_dim}) is outside the kernel's envelope ({Fh.ATTN_ENVELOPE})")
        self.embed_dim, self.num_heads, self.head_dim = int(embed_dim), int(num_heads), int(head_dim)
        self.dropout = 0.0
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = _OutProj(embed_dim, bias)
        self.spd_buckets = None if spd_buckets is None else int(spd_buckets)
        if self.spd_buckets is not None:        # after every parameter of before: today's state_dict order first
            self.spd_bias = _SPDBias(self.spd_buckets, self.num_heads)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """torch's scheme in torch's order of draws (out_proj is built as a Linear first, then
        ``MultiheadAttention._reset_parameters``): the same generator state gives the same weights."""
        nn.init.kaiming_uniform_(self.out_proj.weight, a=math.sqrt(5))
        if self.out_proj.bias is not None:
            bound = 1.0 / math.sqrt(self.embed_dim)
            nn.init.uniform_(self.out_proj.bias, -bound, bound)          # (Linear's draw; zeroed below, as torch does)
        nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            nn.init.constant_(self.in_proj_bias, 0.0)
            nn.init.constant_(self.out_proj.bias, 0.0)
        if self.spd_buckets is not None:        # drawn last: the draws above are those of a module without the table
            nn.init.normal_(self.spd_bias.weight, mean=0.0, std=0.02)

    def forward(self, x: Tensor, batch=None, *, ptr32: Optional[Tensor] = None, max_nodes: Optional[int] = None,
                need_weights: bool = False, attn_mask=None, key_padding_mask=None, attn_bias=None, spd=None) -> Tensor:
        if need_weights:
            raise NotImplementedError("MultiheadSelfAttention(need_weights=True): the attention weights are streamed "
                                      "through LDS and never exist in memory")
        for name, v in (("attn_mask", attn_mask), ("key_padding_mask", key_padding_mask), ("attn_bias", attn_bias)):
            if v is not None:
                raise NotImplementedError(f"MultiheadSelfAttention({name}=...): the only mask is the graph boundary "
                                          "(ptr32); attention bias and other masks are not implemented")
        if batch is not None:
            if ptr32 is not None or max_nodes is not None:
                raise ValueError("pass a Batch, or ptr32 and max_nodes, not both")
            for attr in ("ptr32", "max_nodes"):
                if not hasattr(batch, attr):
                    raise ValueError(f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)")
            ptr32, max_nodes = batch.ptr32, batch.max_nodes
        if ptr32 is None or max_nodes is None:
            raise ValueError("MultiheadSelfAttention needs the graph boundaries: a Batch, or ptr32 and max_nodes")
        if x.dim() != 2 or x.size(1) != self.embed_dim:
            raise ValueError(f"x must be [N, {self.embed_dim}], got {tuple(x.shape)}")
        if self.spd_buckets is None:
            if spd is not None:
                raise ValueError("MultiheadSelfAttention(spd=...): this module has no shortest-path bias table; build "
                                 "it with spd_buckets=max_dist + 1")
        else:
            if not isinstance(spd, Fh.SPDBuckets):
                raise ValueError(f"MultiheadSelfAttention(spd_buckets={self.spd_buckets}) needs spd=: the SPDBuckets "
                                 "of this batch (nn.functional.shortest_path_buckets)")
            if spd.num_buckets != self.spd_buckets:
                raise ValueError(f"MultiheadSelfAttention: spd has max_dist + 1 = {spd.num_buckets} buckets, the "
                                 f"module's table has spd_buckets = {self.spd_buckets}")
        qkv = Fh.linear_wide(x, self.in_proj_weight, self.in_proj_bias)
        if self.spd_buckets is None:
            out = Fh.SelfAttentionFn.apply(qkv, ptr32, int(max_nodes), self.num_heads)
        else:
            out = Fh.BiasedSelfAttentionFn.apply(qkv, self.spd_bias.weight, spd, ptr32, int(max_nodes), self.num_heads)
        return self.out_proj(out)


class _Proj(nn.Module):
    """A ``Linear(channels, channels)`` of ``ExphormerAttention`` (torch's ``nn.Linear`` keys and initialisation),
    through ``linear_wide``."""

    def __init__(self, channels: int, bias: bool):
        super().__init__()
        self.in_features = self.out_features = channels
        self.weight = nn.Parameter(torch.empty(channels, channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(channels))
        else:
            self.register_parameter("bias", None)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if bias:
            bound = 1.0 / math.sqrt(channels)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x: Tensor) -> Tensor:
        return Fh.linear_wide(x, self.weight, self.bias)


class ExphormerAttention(nn.Module):
    """Exphormer's sparse attention (Shirzad et al., "Exphormer: Sparse Transformers for Graphs", 2023) over the union
    of a batch's own edges, an expander and ``num_virtual_nodes`` virtual nodes per graph
    (``structure.ExphormerStructure``), on the HIP path (csrc/exphormer.hip).

    ``forward(x, struct, e_edge, e_type)``: ``x`` [N + B nv, channels] -- the node rows, then the virtual rows;
    ``e_edge`` [E_local, channels] the encoded features of the local edges (None when the structure names none);
    ``e_type`` [2 + 2 nv, channels] the edge-type embeddings.  ``Q``, ``K``, ``V`` project ``x``; ``E`` projects
    ``e_edge`` and ``e_type`` alike, so the typed edges cost T rows of GEMM, not E_union.  Returns
    ``(out_proj(attention[:N]), attention[N:])``: the virtual rows leave the layer as the raw attention output.

    Not provided: dropout on the attention weights, a shortest-path bias, CPU tensors."""

    def __init__(self, channels: int, num_heads: int, num_virtual_nodes: int, use_bias: bool = False):
        super().__init__()
        if channels <= 0 or num_heads <= 0 or channels % num_heads:
            raise ValueError(f"channels must be a positive multiple of num_heads, got channels={channels} and "
                             f"num_heads={num_heads}")
        if not 0 <= int(num_virtual_nodes) <= Fh.EXPH_MAX_VIRTUAL_NODES:
            raise ValueError(f"num_virtual_nodes must be in [0, {Fh.EXPH_MAX_VIRTUAL_NODES}], got {num_virtual_nodes}")
        if channels > Fh.EXPH_MAX_WIDTH:
            raise ValueError(f"ExphormerAttention: channels={channels} is outside the kernel's envelope "
                             f"({Fh.EXPH_ENVELOPE})")
        self.channels, self.num_heads, self.num_virtual_nodes = int(channels), int(num_heads), int(num_virtual_nodes)
        self.Q = _Proj(channels, use_bias)
        self.K = _Proj(channels, use_bias)
        self.V = _Proj(channels, use_bias)
        self.E = _Proj(channels, use_bias)
        self.out_proj = _Proj(channels, True)

    def forward(self, x: Tensor, struct, e_edge: Optional[Tensor], e_type: Tensor):
        if x.dim() != 2 or x.size(1) != self.channels:
            raise ValueError(f"x must be [N + B * nv, {self.channels}], got {tuple(x.shape)}")
        if struct.num_virtual_nodes != self.num_virtual_nodes:
            raise ValueError(f"the structure has {struct.num_virtual_nodes} virtual nodes per graph, the module "
                             f"{self.num_virtual_nodes}")
        ee = None if e_edge is None else self.E(e_edge)
        out = Fh.ExphormerAttentionFn.apply(self.Q(x), self.K(x), self.V(x), ee, self.E(e_type), struct, self.num_heads)
        N = struct.num_nodes
        return self.out_proj(out[:N]), out[N:]


class SANAttention(nn.Module):
    """SAN's multi-head attention (Kreuzer et al., "Rethinking Graph Transformers with Spectral Attention", 2021, in
    GraphGPS's ``SANLayer`` form) on the HIP path (csrc/san.hip): every node attends to its in-neighbours through ``Q``,
    ``K`` and the edge features ``E(edge_attr)``, and -- with ``full_graph`` -- to every other node of its graph (itself
    included, unless it has a self-loop) through ``Q_2``, ``K_2`` and ``E_2`` of ONE learned "fake edge" row; the two
    kinds are mixed by ``gamma`` under one denominator (``nn.functional.SANAttentionFn``).  ``V`` serves both kinds.
    All projections are bias-free ``channels -> channels`` Linears under GraphGPS's names.

    ``forward(x, edge_index, edge_attr, batch, fake_edge_row)``: ``x`` [N, channels], ``edge_attr`` [E, channels] (the
    encoded edge features, one row per edge), ``batch`` the ``Batch`` (``ptr32``, ``max_nodes``; or ``ptr32=`` and
    ``max_nodes=``), ``fake_edge_row`` [1, channels] the model's ``fake_edge_emb.weight`` (read with ``full_graph``
    only).  ``K_2(x) * E_2(fake_edge_row)`` is a row broadcast in plain torch, so autograd carries ``K_2``, ``E_2`` and
    the row.  Returns [N, channels]: the heads side by side, no output projection (the layer's ``O_h`` follows).

    Not provided, refused by name: a learned gamma (``gamma_learn``), dropout on the attention weights, a batch without
    edge features, widths outside the kernel's envelope, CPU tensors."""

    def __init__(self, channels: int, num_heads: int, gamma: float = 1e-1, full_graph: bool = True,
                 attn_dropout: float = 0.0, gamma_learn: bool = False):
        super().__init__()
        if channels <= 0 or num_heads <= 0 or channels % num_heads:
            raise ValueError(f"channels must be a positive multiple of num_heads, got channels={channels} and "
                             f"num_heads={num_heads}")
        if gamma_learn:
            raise NotImplementedError("SANAttention(gamma_learn=True): a learned gamma is not implemented; gamma is a "
                                      "fixed hyperparameter")
        if attn_dropout != 0.0:
            raise NotImplementedError("SANAttention(attn_dropout > 0): dropout on the attention weights is not "
                                      "implemented (the weights never exist in memory); drop the layer's output instead")
        head_dim = channels // num_heads
        if not (head_dim % 4 == 0 and Fh.SAN_MIN_HEAD_DIM <= head_dim <= Fh.SAN_MAX_HEAD_DIM
                and channels <= Fh.SAN_MAX_WIDTH):
            raise ValueError(f"SANAttention: channels={channels} with num_heads={num_heads} (head width {head_dim}) is "
                             f"outside the kernel's envelope ({Fh.SAN_ENVELOPE})")
        self.channels, self.num_heads = int(channels), int(num_heads)
        self.full_graph = bool(full_graph)
        self.gamma = Fh._check_gamma(gamma)
        self.Q = _Proj(channels, False)
        self.K = _Proj(channels, False)
        self.E = _Proj(channels, False)
        if self.full_graph:
            self.Q_2 = _Proj(channels, False)
            self.K_2 = _Proj(channels, False)
            self.E_2 = _Proj(channels, False)
        self.V = _Proj(channels, False)

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor], batch=None,
                fake_edge_row: Optional[Tensor] = None, *, ptr32: Optional[Tensor] = None,
                max_nodes: Optional[int] = None) -> Tensor:
        from ..structure import relation_of
        if x.dim() != 2 or x.size(1) != self.channels:
            raise ValueError(f"x must be [N, {self.channels}], got {tuple(x.shape)}")
        if edge_attr is None:
            raise ValueError("SANAttention needs edge_attr [E, channels]: the real pairs' score is multiplicative in "
                             "the edge features (a batch without edge features is not taken)")
        if edge_attr.dim() != 2 or edge_attr.size(0) != edge_index.size(1) or edge_attr.size(1) != self.channels:
            raise ValueError(f"edge_attr must be [E, {self.channels}] with one row per edge (E = {edge_index.size(1)}), "
                             f"got {tuple(edge_attr.shape)}")
        if batch is not None:
            if ptr32 is not None or max_nodes is not None:
                raise ValueError("pass a Batch, or ptr32 and max_nodes, not both")
            for attr in ("ptr32", "max_nodes"):
                if not hasattr(batch, attr):
                    raise ValueError(f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)")
            ptr32, max_nodes = batch.ptr32, batch.max_nodes
        if ptr32 is None or max_nodes is None:
            raise ValueError("SANAttention needs the graph boundaries: a Batch, or ptr32 and max_nodes")
        q2 = k2e = None
        if self.full_graph:
            if fake_edge_row is None or tuple(fake_edge_row.shape) != (1, self.channels):
                raise ValueError(f"SANAttention(full_graph=True) needs fake_edge_row [1, {self.channels}] (the model's "
                                 "fake_edge_emb.weight)")
            q2 = self.Q_2(x)
            k2e = self.K_2(x) * self.E_2(fake_edge_row)
        rel = relation_of(edge_index, x.size(0), x.size(0))
        out, _ = Fh.SANAttentionFn.apply(self.Q(x), self.K(x), self.V(x), self.E(edge_attr), q2, k2e, rel, ptr32,
                                         int(max_nodes), self.num_heads, self.gamma, self.full_graph)
        return out
