"""Plain-torch restatement of SAN's pieces (CPU, a caller-chosen float dtype): the attention over real and fake pairs,
the layer and the model.  There is no published copy to compare with here: THIS file and the issue's definition are
what the HIP path (csrc/san.hip, nn/attention.py SANAttention, nn/san.py, model/san.py) is held to.

  real   every edge x = (j -> i) of edge_index with both ends in i's graph, each listed edge once:
           s_x = sum_c q[i,c] k[j,c] e[x,c] / sqrt(C)          w_x = a exp(clamp(s_x, -5, 5))
  fake   every node j of i's graph, j = i included, for which no edge j -> i is listed:
           s2_ij = sum_c q2[i,c] k2e[j,c] / sqrt(C)            w2_ij = b exp(clamp(s2_ij, -5, 5))
  a = 1 / (1 + gamma), b = gamma / (1 + gamma);  full_graph = False: the real term alone with a = 1
  Z_i = sum w_x + sum w2_ij        out_i = (sum w_x v_j + sum w2_ij v_j) / (Z_i + 1e-6)

The attention walks every target i of every graph and, for it, every node j of the graph: whether (j, i) is real is
decided by SCANNING THE EDGE LIST for that pair (no CSR, no bitset, no adjacency matrix: nothing the kernel builds), a
pair listed m times giving m real terms.  Slow and obvious on purpose."""
import math

import torch
import torch.nn as nn

CLAMP, EPS = 5.0, 1e-6


def mixing(gamma, full_graph=True):
    return (1.0 / (1.0 + gamma), gamma / (1.0 + gamma)) if full_graph else (1.0, 0.0)


def pairs(edge_index, ptr):
    """For every graph g and every target i of it: (i, [(j, [edge ids of j -> i, in list order]) for j in the graph])."""
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    ptr = [int(p) for p in ptr]
    out = []
    for g in range(len(ptr) - 1):
        lo, hi = ptr[g], ptr[g + 1]
        for i in range(lo, hi):
            into_i = [x for x in range(len(dst)) if dst[x] == i]         # one scan of the list per target
            out.append((i, [(j, [x for x in into_i if src[x] == j]) for j in range(lo, hi)]))
    return out


def attention(q, k, v, e, q2, k2e, edge_index, ptr, heads, gamma=0.1, full_graph=True, skip=None, want_scores=False):
    """-> (out [N, HC], Z [N, heads]).  ``skip``: ("real", x) leaves the term of edge x out (the pair does not turn
    fake); ("fake", (j, i)) leaves the fake term of the ordered pair j -> i out.  ``want_scores``: also the unclamped
    scores, (real [.., heads], fake [.., heads])."""
    N, HC = q.shape
    C = HC // heads
    a, b = mixing(gamma, full_graph)
    rs = 1.0 / math.sqrt(C)
    outs, zs, s_real, s_fake = [None] * N, [None] * N, [], []
    for i, row in pairs(edge_index, ptr):
        real_x, real_j, fake_j = [], [], []
        for j, ids in row:                                              # every ordered pair (j, i) of the graph
            for x in ids:                                               # real: one term per listed edge
                if skip != ("real", x):
                    real_x.append(x), real_j.append(j)
            if not ids and full_graph and skip != ("fake", (j, i)):     # fake: no edge j -> i is listed
                fake_j.append(j)
        Z = torch.zeros(heads, dtype=q.dtype)
        num = torch.zeros(heads, C, dtype=q.dtype)
        if real_x:                                                      # the row's terms of a kind, summed at once
            s = (q[i].view(1, heads, C) * k[real_j].view(-1, heads, C) * e[real_x].view(-1, heads, C)).sum(-1) * rs
            s_real.append(s)
            w = a * torch.exp(s.clamp(-CLAMP, CLAMP))
            Z = Z + w.sum(0)
            num = num + (w.unsqueeze(-1) * v[real_j].view(-1, heads, C)).sum(0)
        if fake_j:
            s = (q2[i].view(1, heads, C) * k2e[fake_j].view(-1, heads, C)).sum(-1) * rs
            s_fake.append(s)
            w = b * torch.exp(s.clamp(-CLAMP, CLAMP))
            Z = Z + w.sum(0)
            num = num + (w.unsqueeze(-1) * v[fake_j].view(-1, heads, C)).sum(0)
        outs[i], zs[i] = (num / (Z + EPS).unsqueeze(-1)).reshape(HC), Z
    for i in range(N):                                                  # rows outside every graph of ptr
        if outs[i] is None:
            outs[i], zs[i] = torch.zeros(HC, dtype=q.dtype), torch.zeros(heads, dtype=q.dtype)
    out = torch.stack(outs) if N else q.new_zeros(0, HC)
    Z = torch.stack(zs) if N else q.new_zeros(0, heads)
    if want_scores:
        stack = lambda l: torch.cat(l) if l else q.new_zeros(0, heads)
        return out, Z, stack(s_real), stack(s_fake)
    return out, Z


class SANAttentionRef(nn.Module):
    def __init__(self, D, heads, gamma=0.1, full_graph=True):
        super().__init__()
        self.heads, self.gamma, self.full_graph = heads, gamma, full_graph
        self.Q, self.K, self.E = (nn.Linear(D, D, bias=False) for _ in range(3))
        if full_graph:
            self.Q_2, self.K_2, self.E_2 = (nn.Linear(D, D, bias=False) for _ in range(3))
        self.V = nn.Linear(D, D, bias=False)

    def forward(self, x, edge_index, edge_attr, ptr, fake_row, skip=None):
        q2 = k2e = None
        if self.full_graph:
            q2, k2e = self.Q_2(x), self.K_2(x) * self.E_2(fake_row)
        return attention(self.Q(x), self.K(x), self.V(x), self.E(edge_attr), q2, k2e, edge_index, ptr, self.heads,
                         self.gamma, self.full_graph, skip)[0]


def _norm(kind, D):
    return nn.LayerNorm(D) if kind == "layer" else (nn.BatchNorm1d(D) if kind == "batch" else None)


class SANLayerRef(nn.Module):
    def __init__(self, D, heads, gamma=0.1, full_graph=True, norm="layer"):
        super().__init__()
        self.attention = SANAttentionRef(D, heads, gamma, full_graph)
        self.O_h = nn.Linear(D, D)
        self.norm1_h = _norm(norm, D)
        self.FFN_h_layer1 = nn.Linear(D, 2 * D)
        self.FFN_h_layer2 = nn.Linear(2 * D, D)
        self.norm2_h = _norm(norm, D)
        self.watch = None

    def set_watch(self, watch, prefix=""):
        self.watch = None if watch is None else (lambda tag, t: watch(prefix + tag, t))

    def forward(self, x, edge_index, edge_attr, ptr, fake_row=None, skip=None):
        h = x + self.O_h(self.attention(x, edge_index, edge_attr, ptr, fake_row, skip))
        if self.norm1_h is not None:
            h = self.norm1_h(h)
        f = self.FFN_h_layer1(h)
        if self.watch is not None:
            self.watch("feed-forward hidden layer", f)
        h = h + self.FFN_h_layer2(torch.relu(f))
        if self.norm2_h is not None:
            h = self.norm2_h(h)
        return h


class CategoricalRef(nn.Module):
    """OGB's Atom / BondEncoder with its tables in one ``weight`` (encoder/categorical.py): sum_c weight[off_c + x[:, c]]."""

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


class LapPERef(nn.Module):
    """encoder/lappe.py LapPENodeEncoder's ``pe`` (DeepSet, no sign flip): per (node, frequency) the pair (vec, val),
    NaN read as 0, through Linear + ReLU layers; the frequencies whose vec is not NaN summed; Linear + ReLU post layers."""

    def __init__(self, dim_pe, layers, post_layers):
        super().__init__()
        w = [2] + [2 * dim_pe] * (layers - 1) + [dim_pe]
        self.linear_A = nn.Linear(w[0], w[1])
        self.pe_encoder = nn.ModuleList(nn.Linear(i, o) for i, o in zip(w[1:-1], w[2:]))
        pw = [dim_pe] + [2 * dim_pe] * (post_layers - 1) + [dim_pe] if post_layers > 0 else [dim_pe]
        self.post_mlp = nn.ModuleList(nn.Linear(i, o) for i, o in zip(pw[:-1], pw[1:]))
        self.watch = None

    def pe(self, vec, val):
        val = val.squeeze(2) if val.dim() == 3 else val
        live = ~torch.isnan(vec)
        a = torch.stack([torch.nan_to_num(vec, nan=0.0), torch.nan_to_num(val, nan=0.0)], -1)
        for n, fc in enumerate([self.linear_A] + list(self.pe_encoder)):
            a = fc(a)
            if self.watch is not None:
                self.watch(f"LapPE layer {n}", a[live])
            a = torch.relu(a)
        pe = (a * live.unsqueeze(-1).to(a.dtype)).sum(1)
        for n, fc in enumerate(self.post_mlp):
            pe = fc(pe)
            if self.watch is not None:
                self.watch(f"LapPE post layer {n}", pe)
            pe = torch.relu(pe)
        return pe


class SANRef(nn.Module):
    """model/san.py SAN.  ``node_encoder`` / ``edge_encoder``: None (a Linear of ``F`` / ``edge_dim`` float columns) or
    the cardinalities of a categorical encoder; ``lappe = (dim_pe, layers, post_layers)`` or None."""

    def __init__(self, F, D, C, L, heads, gamma=0.1, full_graph=True, task_level="graph", edge_dim=None,
                 node_encoder=None, edge_encoder=None, lappe=None, norm="layer"):
        super().__init__()
        self.task_level, self.full_graph = task_level, full_graph
        Dx = D - (lappe[0] if lappe else 0)
        self.node_encoder = nn.Linear(F, Dx) if node_encoder is None else CategoricalRef(node_encoder, Dx)
        self.edge_encoder = nn.Linear(edge_dim, D) if edge_encoder is None else CategoricalRef(edge_encoder, D)
        if full_graph:
            self.fake_edge_emb = nn.Embedding(1, D)
        self.layers = nn.ModuleList(SANLayerRef(D, heads, gamma, full_graph, norm) for _ in range(L))
        self.lin_1 = nn.Linear(D, D)
        self.lin_2 = nn.Linear(D, C)
        if lappe:
            self.pe_encoder = LapPERef(*lappe)
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch
        for i, layer in enumerate(self.layers):
            layer.set_watch(watch, f"layer {i} ")
        if hasattr(self, "pe_encoder"):
            self.pe_encoder.watch = watch

    def forward(self, x, edge_index, edge_attr, batch, ptr, pairs=None, stats=None, skip=None):
        """``stats = (vec, val)`` for a model with ``lappe``; ``skip``: a term left out of every layer's attention."""
        num_graphs = len(ptr) - 1
        h = self.node_encoder(x)
        if hasattr(self, "pe_encoder"):
            h = torch.cat((h, self.pe_encoder.pe(*stats)), 1)
        e = self.edge_encoder(edge_attr)
        fake = self.fake_edge_emb.weight if self.full_graph else None
        for layer in self.layers:
            h = layer(h, edge_index, e, ptr, fake, skip)
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
