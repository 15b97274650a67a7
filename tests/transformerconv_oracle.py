"""Plain-torch restatement of TransformerConv (multi-head scaled dot-product attention over the in-edges of every node,
optional edge features added to keys and values), written from the formulas (CPU, any float dtype).  With
j = edge_index[0, k] the source and i = edge_index[1, k] the target of edge k, ``Hd`` heads of width ``C``:

    s_k   = sum_c q[i,h,c] * (k[j,h,c] + e[k,h,c]) / sqrt(C)
    a_k   = exp(s_k) / sum_{k': dst_k' = i} exp(s_k')            per head (the row maximum is subtracted first)
    out_i = sum_{k: dst_k = i} a_k * (v[j,h,:] + e[k,h,:])        (0 for a node without in-edges)

every edge as given: loops and repeated edges count.  The float32 and float64 evaluations of these functions and modules
are the two oracles of tests/test_gpu_transformerconv.py; ``skip`` removes one edge from the softmax and the sum (the
toothed variant).  Module and parameter names are the product's (PyG's), so a ``state_dict`` moves across.
``watch(tag, tensor)`` receives every ReLU input for the kink guard -- the operator itself is smooth."""
import math

import torch
import torch.nn as nn

LL, VV, LV = ("local", "to", "local"), ("virtual", "to", "virtual"), ("local", "to", "virtual")


def aggregate(q, k, v, e, edge_index, heads, skip=None):
    """out [Nd, Hd*C]; ``e`` [E, Hd*C] or None; ``skip``: an edge number left out."""
    Nd, HC = q.shape
    C = HC // heads
    src, dst = edge_index[0], edge_index[1]
    E = src.numel()
    if skip is not None:
        keep = torch.ones(E, dtype=torch.bool)
        keep[skip] = False
        src, dst = src[keep], dst[keep]
        e = e[keep] if e is not None else None
    kk, vv = k[src], v[src]
    if e is not None:
        kk, vv = kk + e, vv + e
    kk, vv = kk.view(-1, heads, C), vv.view(-1, heads, C)
    s = (q[dst].view(-1, heads, C) * kk).sum(-1) * (1.0 / math.sqrt(C))                # [E, Hd]
    m = torch.full((Nd, heads), -math.inf, dtype=q.dtype)
    m = m.scatter_reduce(0, dst.unsqueeze(1).expand(-1, heads), s.detach(), "amax", include_self=True)
    w = torch.exp(s - m[dst])
    den = torch.zeros(Nd, heads, dtype=q.dtype).index_add_(0, dst, w)
    a = w / den[dst]
    return torch.zeros(Nd, heads, C, dtype=q.dtype).index_add_(0, dst, a.unsqueeze(-1) * vv).view(Nd, HC)


def dense(q, k, v, edge_index, heads):
    """The same without edge features, restated densely and independently: with M[i, j] the number of edges j -> i,
    ``out_i = sum_j M_ij exp(s_ij) v_j / sum_j M_ij exp(s_ij)`` per head, over all (target, source) pairs."""
    Nd, HC = q.shape
    Ns, C = k.size(0), HC // heads
    M = torch.zeros(Nd, Ns, dtype=q.dtype)
    M.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.size(1), dtype=q.dtype), accumulate=True)
    out = torch.zeros(Nd, heads, C, dtype=q.dtype)
    for h in range(heads):
        qh, kh, vh = (t.view(-1, heads, C)[:, h] for t in (q, k, v))
        s = qh @ kh.t() / math.sqrt(C)
        s = s.masked_fill(M == 0, -math.inf)
        top = s.max(1, keepdim=True).values
        top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
        w = M * torch.exp(s - top)
        den = w.sum(1, keepdim=True)
        out[:, h] = torch.where(den > 0, w / den.clamp(min=1e-300), torch.zeros_like(w)) @ vh
    return out.view(Nd, HC)


def most_changing_edge(q, k, v, e, edge_index, heads):
    """The edge whose removal changes ``out`` most (max norm) among the rows with more than one edge: the one with the
    largest a_k |v_j + e_k - out_i| / (1 - a_k) -- removing edge k from a row moves out_i by exactly that -- found
    without E evaluations.  The only edge of a row (a_k = 1; its removal empties the row, which moves by |out_i|) is a
    candidate only where every row has one edge: the softmax over one logit does not depend on q or k, so its removal
    would not reach their gradients."""
    Nd, HC = q.shape
    C = HC // heads
    src, dst = edge_index[0], edge_index[1]
    kk, vv = k[src], v[src]
    if e is not None:
        kk, vv = kk + e, vv + e
    s = (q[dst].view(-1, heads, C) * kk.view(-1, heads, C)).sum(-1) / math.sqrt(C)
    m = torch.full((Nd, heads), -math.inf, dtype=q.dtype).scatter_reduce(
        0, dst.unsqueeze(1).expand(-1, heads), s, "amax", include_self=True)
    w = torch.exp(s - m[dst])
    a = w / torch.zeros(Nd, heads, dtype=q.dtype).index_add_(0, dst, w)[dst]
    out = aggregate(q, k, v, e, edge_index, heads).view(Nd, heads, C)
    diff = (vv.view(-1, heads, C) - out[dst]).abs().amax(-1)
    alone = a >= 1.0 - 1e-12
    move = torch.where(alone, torch.zeros_like(a), a * diff / (1.0 - a).clamp(min=1e-300))
    if bool(alone.all()):
        move = out[dst].abs().amax(-1)
    return int(move.amax(1).argmax())


class TransformerConvRef(nn.Module):
    """``lin_key`` / ``lin_query`` / ``lin_value`` with bias, ``lin_edge`` without (only with ``edge_dim``), ``lin_skip``
    (only with ``root_weight``); ``in_channels``: an int or a pair (source width, target width)."""

    def __init__(self, in_channels, out_channels, heads=1, edge_dim=None, bias=True, root_weight=True):
        super().__init__()
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.heads, self.out_channels = heads, out_channels
        width = heads * out_channels
        self.lin_key = nn.Linear(in_channels[0], width)
        self.lin_query = nn.Linear(in_channels[1], width)
        self.lin_value = nn.Linear(in_channels[0], width)
        self.lin_edge = nn.Linear(edge_dim, width, bias=False) if edge_dim is not None else None
        self.lin_skip = nn.Linear(in_channels[1], width, bias=bias) if root_weight else None
        self.watch = None

    def forward(self, x, edge_index, edge_attr=None, act="identity", skip=None):
        x_src, x_dst = (x, x) if isinstance(x, torch.Tensor) else x
        e = self.lin_edge(edge_attr) if self.lin_edge is not None else None
        out = aggregate(self.lin_query(x_dst), self.lin_key(x_src), self.lin_value(x_src), e, edge_index, self.heads, skip)
        if self.lin_skip is not None:
            out = out + self.lin_skip(x_dst)
        if act == "relu":
            if self.watch is not None:
                self.watch("output", out)
            out = torch.relu(out)
        return out


def _pool(x, batch, num_graphs):
    sums = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
    return sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)


class BondRef(nn.Module):
    """The product's BondEncoder restated: one table ``weight [sum(cards), H]``, column c owning the rows from
    ``sum(cards[:c])``; int64 categories [E, F] -> the sum over columns of their rows, in column order."""

    def __init__(self, cards, H):
        super().__init__()
        self.offsets = [sum(cards[:c]) for c in range(len(cards))]
        self.weight = nn.Parameter(torch.empty(sum(cards), H))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, x):
        out = self.weight[self.offsets[0] + x[:, 0]]
        for c in range(1, x.size(1)):
            out = out + self.weight[self.offsets[c] + x[:, c]]
        return out


class MPNNRef(nn.Module):
    """The MPNN baseline with conv = TransformerConv: L layers F -> heads x (H / heads) -> ... -> 1 x C, ReLU after every
    hidden layer; then the per-graph mean ("graph"), the node outputs ("node") or the dot product of candidate pairs
    ("link").  ``edge_dim``: every layer reads the same ``edge_attr`` through its own ``lin_edge``; ``bond_cards``: a
    ``BondRef`` of width H in front of them."""

    def __init__(self, F, H, C, L, heads, edge_dim=None, task_level="graph", bond_cards=None):
        super().__init__()
        if bond_cards is not None:
            self.edge_encoder = BondRef(bond_cards, H)
            edge_dim = H
        dims = [(F, H // heads, heads)] + [(H, H // heads, heads)] * (L - 2) + [(H, C, 1)]
        self.conv_layers = nn.ModuleList(TransformerConvRef(i, o, h, edge_dim) for i, o, h in dims)
        self.task_level = task_level
        self.bond = bond_cards is not None

    def set_watch(self, watch):
        for i, c in enumerate(self.conv_layers):
            c.watch = None if watch is None else (lambda tag, t, i=i: watch(f"layer {i} {tag}", t))

    def forward(self, x, edge_index, edge_attr, batch, num_graphs, pairs=None, skip=None):
        if self.bond:
            edge_attr = self.edge_encoder(edge_attr)
        for c in self.conv_layers[:-1]:
            x = c(x, edge_index, edge_attr, "relu", skip)
        x = self.conv_layers[-1](x, edge_index, edge_attr, "identity", skip)
        if self.task_level == "node":
            return x
        if self.task_level == "link":
            return (x[pairs[0]] * x[pairs[1]]).sum(1)
        return _pool(x, batch, num_graphs)


def gps_twin(F, D, C, L, heads, edge_dim):
    """tests/gps_oracle.py's GPS with the local branch ``x + TransformerConv(x, e)``: heads of width D / heads."""
    from tests import gps_oracle as GP

    class Layer(GP.GPSLayerRef):
        def __init__(self):
            super().__init__(D, None, heads, "layer")
            self.local_conv = "transformerconv_edge"
            self.conv = TransformerConvRef(D, D // heads, heads, edge_dim)
            self.norm1_local = GP._norm("layer", D)
            self.edge_skip = None

        def forward(self, x, edge_index, ptr, edge_attr=None, skip=None):
            h_a = self.norm1_attn(x + self.attn(x, ptr, skip))
            h_l = self.norm1_local(x + self.conv(x, edge_index, edge_attr, skip=self.edge_skip))
            h = h_l + h_a
            f = self.ff_linear1(h)
            if self.watch is not None:
                self.watch("feed-forward hidden layer", f)
            return self.norm2(h + self.ff_linear2(torch.relu(f)))

    m = GP.GPSRef(F, D, C, 0, heads, None, "layer", "graph")
    m.layers = nn.ModuleList(Layer() for _ in range(L))
    return m


class _Hetero(nn.Module):
    def __init__(self, convs):
        super().__init__()
        self.convs = nn.ModuleDict({"__".join(k): v for k, v in convs.items()})


class HSCNRef(nn.Module):
    """HSCN with lv = ll = vv = TransformerConv: per layer the three relations in ``edge_index_dict`` order, outputs
    that share a target type summed, a hard ReLU on both types; mean pool of the local nodes, lin_2(relu(lin_1))."""

    def __init__(self, F, H, C, L, heads):
        super().__init__()
        self.convs = nn.ModuleList()
        for layer in range(L):
            fin = F if layer == 0 else H
            self.convs.append(_Hetero({k: TransformerConvRef(fin, H // heads, heads) for k in (LV, LL, VV)}))
        self.lin_1 = nn.Linear(H, H)
        self.lin_2 = nn.Linear(H, C)
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch

    def forward(self, x_dict, edge_index_dict, batch_local, num_graphs, skip=None):
        """``skip = (edge type, edge number)``: left out in every layer."""
        for li, conv in enumerate(self.convs):
            outs = {}
            for et, ei in edge_index_dict.items():
                c = conv.convs["__".join(et)]
                x = x_dict[et[0]] if et[0] == et[2] else (x_dict[et[0]], x_dict[et[2]])
                outs.setdefault(et[2], []).append(c(x, ei, skip=skip[1] if skip is not None and skip[0] == et else None))
            x_dict = {k: (v[0] if len(v) == 1 else torch.stack(v, 0).sum(0)) for k, v in outs.items()}
            if self.watch is not None:
                for k, v in x_dict.items():
                    self.watch(f"layer {li} {k}", v)
            x_dict = {k: v.relu() for k, v in x_dict.items()}
        h = self.lin_1(_pool(x_dict["local"], batch_local, num_graphs))
        if self.watch is not None:
            self.watch("head hidden layer", h)
        return self.lin_2(torch.relu(h))
