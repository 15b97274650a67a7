"""Plain-torch restatement of Exphormer's pieces (CPU, a caller-chosen float dtype): the expander in numpy with its own
copy of the Philox reference (the style of tests/test_gpu_exact_edges.py), the union graph with its typed feature rows,
the attention, the layer and the model.  There is no published copy of the layer to compare with here: THIS file is the
definition the HIP path is held to.

  expander   cycle r of graph g: node t has key (philox4x32_10(seed, ctr)[0] << 32) | t with
             ctr = (gid << 32) | (r << 16) | t, gid = graph_ids[g] or g; pi = ascending key order; block r is
             pi[i] -> pi[(i + 1) % n] for i = 0..n-1, then the reverses; graph g's n * degree edges start at degree * ptr[g]
  union      local edges (add_local_edges), expander edges, then node i -> virtual t at i * nv + t of one block and
             virtual t -> node i at the same place of the next; virtual row of (g, t) = N + g * nv + t
  erow       < El: row of the per-edge tensor;  El + tau: type tau (0 local without features, 1 expander, 2 + t node ->
             virtual t, 2 + nv + t virtual t -> node)
  attention  s_k = <q_i, k_j * e_k> / sqrt(C) per head, w_k = exp(clamp(s_k, -5, 5)), out_i = sum w_k v_j / (sum w_k + 1e-6)
  layer      attention over cat(x, virt): node rows through out_proj into the GPS layer's attention branch, virtual rows
             out raw
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests import gps_oracle as GP

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
CLAMP, EPS = 5.0, 1e-6


def philox_word0(ctr64, seed):
    """Philox-4x32-10 (Salmon et al., Random123): counter words (ctr low, ctr high, 0, 0), key (seed low, seed high);
    ``ctr64`` a uint64 array -> word 0 of every block, uint64."""
    ctr64 = np.asarray(ctr64, dtype=np.uint64)
    mask = np.uint64(_MASK)
    c0, c1 = ctr64 & mask, ctr64 >> np.uint64(32)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0


def cycle(n, gid, r, seed):
    """pi of cycle r of a graph of n nodes with id gid: the local ids in ascending key order."""
    t = np.arange(n, dtype=np.uint64)
    ctr = (np.uint64(gid) << np.uint64(32)) | (np.uint64(r) << np.uint64(16)) | t
    key = (philox_word0(ctr, seed) << np.uint64(32)) | t
    return np.argsort(key, kind="stable").astype(np.int64)


def expander_edges(sizes, degree, seed, graph_ids=None):
    """int64 tensor [2, degree * N] for graphs of ``sizes`` nodes."""
    assert degree >= 2 and degree % 2 == 0
    N = int(sum(sizes))
    out = np.zeros((2, degree * N), dtype=np.int64)
    lo = 0
    for g, n in enumerate(sizes):
        gid = g if graph_ids is None else int(graph_ids[g])
        for r in range(degree // 2):
            pi = cycle(n, gid, r, seed) + lo
            nxt = np.roll(pi, -1)
            base = degree * lo + 2 * n * r
            out[0, base:base + n], out[1, base:base + n] = pi, nxt
            out[0, base + n:base + 2 * n], out[1, base + n:base + 2 * n] = nxt, pi
        lo += n
    return torch.from_numpy(out)


def union_graph(edge_index, batch_vec, num_graphs, expander, nv, add_local_edges=True, edge_features=True):
    """-> (edge_index_union int64 [2, E], erow int64 [E], El, T, rows)."""
    N, E_local = int(batch_vec.numel()), int(edge_index.size(1))
    El = E_local if (add_local_edges and edge_features) else 0
    src, dst, erow = [], [], []
    if add_local_edges:
        for k in range(E_local):
            src.append(int(edge_index[0, k])), dst.append(int(edge_index[1, k])), erow.append(k if El else El + 0)
    if expander is not None:
        for k in range(int(expander.size(1))):
            src.append(int(expander[0, k])), dst.append(int(expander[1, k])), erow.append(El + 1)
    for direction in (0, 1):
        for i in range(N):
            for t in range(nv):
                virt = N + int(batch_vec[i]) * nv + t
                if direction == 0:
                    src.append(i), dst.append(virt), erow.append(El + 2 + t)
                else:
                    src.append(virt), dst.append(i), erow.append(El + 2 + nv + t)
    ei = torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)
    return ei, torch.tensor(erow, dtype=torch.int64), El, 2 + 2 * nv, N + num_graphs * nv


def edge_rows(e_edge, e_type, erow, El):
    """[E, HC]: every union edge's feature row (what a user would materialise; the HIP path never does)."""
    if El:
        return torch.cat([e_edge, e_type], 0)[erow]
    return e_type[erow - El]


def logits(q, k, e_edge, e_type, edge_index, erow, El, heads):
    """[E, heads] unclamped."""
    E, HC = int(edge_index.size(1)), q.size(1)
    C = HC // heads
    ee = edge_rows(e_edge, e_type, erow, El).view(E, heads, C)
    return (q[edge_index[1]].view(E, heads, C) * k[edge_index[0]].view(E, heads, C) * ee).sum(-1) / math.sqrt(C)


def attention(q, k, v, e_edge, e_type, edge_index, erow, El, heads, skip=None, swap=None):
    """out [rows, HC].  ``skip``: an edge left out; ``swap = (edge, row)``: that edge reads feature row ``row`` instead
    of its own (the toothed variants)."""
    rows, HC = q.shape
    C = HC // heads
    if swap is not None:
        erow = erow.clone()
        erow[swap[0]] = swap[1]
    if skip is not None:
        keep = torch.ones(edge_index.size(1), dtype=torch.bool)
        keep[skip] = False
        edge_index, erow = edge_index[:, keep], erow[keep]
    E = int(edge_index.size(1))
    s = logits(q, k, e_edge, e_type, edge_index, erow, El, heads)
    w = torch.exp(s.clamp(-CLAMP, CLAMP))
    z = torch.zeros(rows, heads, dtype=q.dtype).index_add_(0, edge_index[1], w)
    num = torch.zeros(rows, heads, C, dtype=q.dtype).index_add_(0, edge_index[1],
                                                                 w.unsqueeze(-1) * v[edge_index[0]].view(E, heads, C))
    return (num / (z + EPS).unsqueeze(-1)).reshape(rows, HC)


class ExphormerAttentionRef(nn.Module):
    def __init__(self, D, heads, use_bias=False):
        super().__init__()
        self.heads = heads
        self.Q, self.K, self.V, self.E = (nn.Linear(D, D, bias=use_bias) for _ in range(4))
        self.out_proj = nn.Linear(D, D)

    def forward(self, x, num_nodes, e_edge, e_type, union, skip=None):
        edge_index, erow, El, _, _ = union
        out = attention(self.Q(x), self.K(x), self.V(x), None if e_edge is None else self.E(e_edge), self.E(e_type),
                        edge_index, erow, El, self.heads, skip=skip)
        return self.out_proj(out[:num_nodes]), out[num_nodes:]


class ExphormerLayerRef(GP.GPSLayerRef):
    """``GPSLayerRef`` with the sparse attention in the dense one's place; everything else on the node rows only."""

    def __init__(self, D, local_conv, heads, norm="layer", edge_dim=None):
        super().__init__(D, local_conv, heads, norm, edge_dim)
        self.attn = ExphormerAttentionRef(D, heads)

    def forward(self, x, virt, edge_index, edge_attr, e_edge, e_type, union, skip=None):
        h_a, virt_out = self.attn(torch.cat([x, virt], 0), x.size(0), e_edge, e_type, union, skip)
        h_a = x + h_a
        if self.norm1_attn is not None:
            h_a = self.norm1_attn(h_a)
        h = h_a
        if self.conv is not None:
            h_l = self.conv(x, edge_index, edge_attr) if self.local_conv == "gine" else self.conv(x, edge_index)
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
        return h, virt_out


class _Table(nn.Module):
    def __init__(self, rows, D):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(rows, D))


class ExphormerGPSRef(nn.Module):
    """``GPS(global_model="exphormer")`` with ``local_conv`` None, "gcn" or "gine".  With "gine" the local edges' own
    features reach the attention through ``exph_edge_encoder`` (a Linear of the raw edge_attr to width D)."""

    def __init__(self, F, D, C, L, heads, local_conv, nv, task_level="graph", edge_dim=None, norm="layer"):
        super().__init__()
        self.task_level, self.nv, self.local_conv = task_level, nv, local_conv
        self.node_encoder = nn.Linear(F, D)
        self.layers = nn.ModuleList(ExphormerLayerRef(D, local_conv, heads, norm, edge_dim) for _ in range(L))
        self.lin_1 = nn.Linear(D, D)
        self.lin_2 = nn.Linear(D, C)
        self.virt_node_emb = _Table(nv, D)
        self.edge_type_emb = _Table(2 + 2 * nv, D)
        if local_conv == "gine":
            self.exph_edge_encoder = nn.Linear(edge_dim, D)
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch
        for i, layer in enumerate(self.layers):
            layer.set_watch(watch, f"layer {i} ")

    def forward(self, x, edge_index, edge_attr, batch, num_graphs, union, pairs=None, skip=None):
        """``union``: ``union_graph(...)`` of the batch (edge features present exactly with "gine").  ``skip``: a union
        edge left out of every layer's attention."""
        x = self.node_encoder(x)
        e_edge = self.exph_edge_encoder(edge_attr) if self.local_conv == "gine" else None
        virt = self.virt_node_emb.weight.repeat(num_graphs, 1)
        for layer in self.layers:
            x, virt = layer(x, virt, edge_index, edge_attr, e_edge, self.edge_type_emb.weight, union, skip)
        if self.task_level == "graph":
            sums = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
            x = sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)
        h = self.lin_1(x)
        if self.watch is not None:
            self.watch("head hidden layer", h)
        out = self.lin_2(torch.relu(h))
        if self.task_level == "link":
            return (out[pairs[0]] * out[pairs[1]]).sum(1)
        return out
