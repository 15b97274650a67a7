"""Plain-torch restatement of GCNII (PyG GCN2Conv, LRGB's GCN2ConvLayer form) for tests/test_gcn2_host.py and
tests/test_gpu_gcn2.py: gather with ``index_add_``, products with ``addmm``; float32 or float64 by the dtype of what it
is given.  Nothing here is used by the package.

    A_hat: the edge list without its self loops, one loop per node appended; deg = in-degree of that list;
           weight of edge j -> i = deg_i^-1/2 deg_j^-1/2 (unit edge weights; a repeated edge counts as often as listed)
    p   = A_hat x
    shared:  h = (1 - alpha) p + alpha x0;  y = (1 - beta) h + beta h W1
    two:     y = (1 - beta) ((1 - alpha) p + alpha x0) + beta ((1 - alpha) p W1 + alpha x0 W2)
    out = act(y)

``skip_edge=k``: listed edge k (not a self loop) is left out of the SUM but not of the degrees -- the teeth's missing
term."""
import math

import torch
import torch.nn as nn


def beta_of(theta, layer):
    return 1.0 if theta is None or layer is None else math.log(theta / layer + 1.0)


def with_loops(edge_index, n):
    """(edges with loops appended, listed-edge id of every kept edge)."""
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(n, dtype=torch.long)
    return torch.cat([edge_index[:, keep], torch.stack([loops, loops])], 1), keep.nonzero().flatten()


def propagate(x, edge_index, skip_edge=None):
    """A_hat x over ``edge_index`` [2, E] (listed edges; loops are this function's to add)."""
    n = x.size(0)
    ei, ids = with_loops(edge_index, n)
    src, dst = ei[0], ei[1]
    deg = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=x.dtype))
    dinv = deg.pow(-0.5)
    w = dinv[dst] * dinv[src]
    if skip_edge is not None:
        hit = (ids == int(skip_edge)).nonzero().flatten()
        assert hit.numel() == 1, "skip_edge must name a listed edge that is not a self loop"
        live = torch.ones(src.numel(), dtype=torch.bool)
        live[hit] = False
        src, dst, w = src[live], dst[live], w[live]
    return torch.zeros_like(x).index_add_(0, dst, w.unsqueeze(1) * x[src])


def gcn2(x, x0, edge_index, W1, W2, alpha, beta, act="identity", skip_edge=None):
    p = propagate(x, edge_index, skip_edge)
    x0 = x0[:x.size(0)]
    if W2 is None:
        h = (1.0 - alpha) * p + alpha * x0
        y = torch.addmm(h, h, W1, beta=1.0 - beta, alpha=beta)
    else:
        pa, xa = (1.0 - alpha) * p, alpha * x0
        y = torch.addmm(pa + xa, pa, W1, beta=1.0 - beta, alpha=beta) + beta * (xa @ W2)
    return torch.relu(y) if act == "relu" else y


def glorot_(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-a, a)


class GCN2ConvRef(nn.Module):
    def __init__(self, channels, alpha, theta=None, layer=None, shared_weights=True):
        super().__init__()
        self.alpha, self.beta = float(alpha), beta_of(theta, layer)
        self.weight1 = nn.Parameter(glorot_(torch.empty(channels, channels)))
        if shared_weights:
            self.register_parameter("weight2", None)
        else:
            self.weight2 = nn.Parameter(glorot_(torch.empty(channels, channels)))

    def forward(self, x, x0, edge_index, act="identity", skip_edge=None, pre=None):
        """``pre``: called with the pre-activation (the ReLU's input) when given."""
        y = gcn2(x, x0, edge_index, self.weight1, self.weight2, self.alpha, self.beta, "identity", skip_edge)
        if pre is not None:
            pre(y)
        return torch.relu(y) if act == "relu" else y


class CategoricalRef(nn.Module):
    """OGB's AtomEncoder with its tables in one ``weight`` (encoder/categorical.py): sum_c weight[off_c + x[:, c]]."""

    def __init__(self, cardinalities, D):
        super().__init__()
        self.offsets = [sum(cardinalities[:c]) for c in range(len(cardinalities))]
        self.weight = nn.Parameter(torch.empty(sum(cardinalities), D))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, x):
        out = 0
        for c, off in enumerate(self.offsets):
            out = out + self.weight[off + x[:, c].long()]
        return out


class RWSERef(nn.Module):
    """encoder/rwse.py RWSENodeEncoder's ``pe`` with model="linear": one Linear over the ksteps statistics."""

    def __init__(self, ksteps, dim_pe):
        super().__init__()
        self.pe_encoder = nn.ModuleList([nn.Linear(ksteps, dim_pe)])

    def pe(self, rwse):
        return self.pe_encoder[0](rwse)


class GCNIIRef(nn.Module):
    """model/gcnii.py GCNII.  ``node_encoder``: None (a Linear of ``F`` float columns) or the cardinalities of a
    categorical encoder; ``rwse = (ksteps, dim_pe)`` or None.  ``masks``: per layer a {0, 1} tensor [N, H] and
    ``mask_scale`` = 1 / (1 - p), the dropout the product draws."""

    def __init__(self, F, H, C, L, alpha=0.1, theta=0.5, shared_weights=True, residual=False, task_level="graph",
                 node_encoder=None, rwse=None):
        super().__init__()
        self.task_level, self.residual = task_level, residual
        Hx = H - (rwse[1] if rwse else 0)
        self.node_encoder = nn.Linear(F, Hx) if node_encoder is None else CategoricalRef(node_encoder, Hx)
        self.layers = nn.ModuleList(GCN2ConvRef(H, alpha, theta, l, shared_weights) for l in range(1, L + 1))
        self.lin_1 = nn.Linear(H, H)
        self.lin_2 = nn.Linear(H, C)
        if rwse:
            self.pe_encoder = RWSERef(*rwse)
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch

    def forward(self, x, edge_index, batch, num_graphs, pairs=None, stats=None, skip_edge=None, masks=None,
                mask_scale=1.0):
        h = self.node_encoder(x)
        if hasattr(self, "pe_encoder"):
            h = torch.cat((h, self.pe_encoder.pe(stats)), 1)
        h0 = h
        for l, conv in enumerate(self.layers):
            h_in = h
            pre = None if self.watch is None else (lambda y, l=l: self.watch(f"layer {l + 1} pre-activation", y))
            h = conv(h, h0, edge_index, "relu", skip_edge, pre)
            if masks is not None:
                h = h * masks[l].to(h.dtype) * torch.tensor(mask_scale, dtype=torch.float32).to(h.dtype)
            if self.residual:
                h = h_in + h
        if self.task_level == "graph":
            sums = torch.zeros(num_graphs, h.size(1), dtype=h.dtype).index_add_(0, batch, h)
            h = sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(h.dtype).unsqueeze(1)
        f = self.lin_1(h)
        if self.watch is not None:
            self.watch("head hidden layer", f)
        out = self.lin_2(torch.relu(f))
        if self.task_level == "link":
            return (out[pairs[0]] * out[pairs[1]]).sum(1)
        return out
