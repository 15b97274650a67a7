"""Plain-torch restatement of the GPS layer and model (CPU, any float dtype), built from the existing restatements: the
GCN / GAT convolutions of oracle/pyg_ops.py, GINE of tests/gine_oracle.py, the attention of tests/attention_oracle.py
and torch's own norms and Linears.  Module and parameter names are the product's, so ``state_dict`` moves across.

``watch(tag, tensor)`` receives every ReLU input (feed-forward hidden layers, the head's hidden layer, GINE's message
pre-activations and MLP hidden layers); a GAT convolution keeps its attention logits in ``last_logits``."""
import torch
import torch.nn as nn

from oracle import pyg_ops as P
from tests import attention_oracle as AO
from tests import gine_oracle as GO


class AttentionRef(nn.Module):
    """torch.nn.MultiheadAttention's parameters; the attention itself is the per-graph loop of attention_oracle."""

    def __init__(self, D, heads):
        super().__init__()
        self.heads = heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * D, D))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * D))
        self.out_proj = nn.Linear(D, D)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.normal_(self.in_proj_bias, std=0.1)
        self.term_hook = None                  # optional callable(qkv) per call (the tests' term magnitudes)

    def forward(self, x, ptr, skip=None):
        qkv = x @ self.in_proj_weight.t() + self.in_proj_bias
        if self.term_hook is not None:
            self.term_hook(qkv)
        return self.out_proj(AO.forward(qkv, ptr, self.heads, skip=skip)[0])


def _norm(kind, D):
    return nn.LayerNorm(D) if kind == "layer" else (nn.BatchNorm1d(D) if kind == "batch" else None)


class GPSLayerRef(nn.Module):
    def __init__(self, D, local_conv, heads, norm="layer", edge_dim=None):
        super().__init__()
        self.local_conv = local_conv
        if local_conv == "gcn":
            self.conv = P.GCNConv(D, D)
        elif local_conv == "gat":
            self.conv = P.GATConv((D, D), D)
            self.conv.lin_dst = self.conv.lin_src          # one transform, as PyG builds GATConv(int, out)
        elif local_conv == "gine":
            self.conv = GO.gine_layer(D, D, edge_dim)
        else:
            self.conv = None
        self.attn = AttentionRef(D, heads)
        self.norm1_local = _norm(norm, D) if local_conv is not None else None
        self.norm1_attn = _norm(norm, D)
        self.ff_linear1 = nn.Linear(D, 2 * D)
        self.ff_linear2 = nn.Linear(2 * D, D)
        self.norm2 = _norm(norm, D)
        self.watch = None

    def set_watch(self, watch, prefix=""):
        self.watch = None if watch is None else (lambda tag, t: watch(prefix + tag, t))
        if self.local_conv == "gine":
            self.conv.watch = self.watch

    def forward(self, x, edge_index, ptr, edge_attr=None, skip=None):
        """``skip = (g, j)``: key j of graph g is left out of every attention (the toothed variant)."""
        h_a = x + self.attn(x, ptr, skip)
        if self.norm1_attn is not None:
            h_a = self.norm1_attn(h_a)
        h = h_a
        if self.conv is not None:
            if self.local_conv == "gine":
                h_l = self.conv(x, edge_index, edge_attr)
            elif self.local_conv == "gat":                  # input self loops removed, one loop per node appended
                keep = edge_index[0] != edge_index[1]
                loops = torch.arange(x.size(0)).expand(2, -1)
                h_l = self.conv(x, torch.cat([edge_index[:, keep], loops], 1))
            else:
                h_l = self.conv(x, edge_index)
            h_l = x + h_l
            if self.norm1_local is not None:
                h_l = self.norm1_local(h_l)
            h = h_l + h_a
        f = self.ff_linear1(h)
        if self.watch is not None:
            self.watch("feed-forward hidden layer", f)
        h = h + self.ff_linear2(torch.relu(f))
        if self.norm2 is not None:
            h = self.norm2(h)
        return h


class GPSRef(nn.Module):
    def __init__(self, F, D, C, L, heads, local_conv, norm="layer", task_level="graph", edge_dim=None):
        super().__init__()
        self.task_level = task_level
        self.node_encoder = nn.Linear(F, D)
        self.layers = nn.ModuleList(GPSLayerRef(D, local_conv, heads, norm, edge_dim) for _ in range(L))
        self.lin_1 = nn.Linear(D, D)
        self.lin_2 = nn.Linear(D, C)
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch
        for i, layer in enumerate(self.layers):
            layer.set_watch(watch, f"layer {i} ")

    def forward(self, x, edge_index, edge_attr, batch, ptr, num_graphs, pairs=None, skip=None, pool_skip=None):
        """``pool_skip``: a node left out of the graph-level pool's sum, the count kept (a toothed variant: it reaches
        the tensors in front of the pool whatever the forward values are -- with the count reduced as well, the
        cotangent rows of the graph would still add up to the same total)."""
        x = self.node_encoder(x)
        for layer in self.layers:
            x = layer(x, edge_index, ptr, edge_attr, skip)
        if self.task_level == "graph":
            if pool_skip is not None:
                keep = torch.ones(x.size(0), 1, dtype=x.dtype)
                keep[pool_skip] = 0
                x = x * keep
            sums = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
            x = sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)
        h = self.lin_1(x)
        if self.watch is not None:
            self.watch("head hidden layer", h)
        out = self.lin_2(torch.relu(h))
        if self.task_level == "link":
            return (out[pairs[0]] * out[pairs[1]]).sum(1)
        return out
