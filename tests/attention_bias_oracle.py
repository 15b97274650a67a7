"""Plain-torch restatement of the shortest-path buckets and of the self-attention they bias (CPU, float32 or float64),
written from the formulas:

    bucket(i, j) = min(d(i, j), max_dist),  d = the fewest edges on a directed path i -> j inside the graph (BFS)
    S = scale Q K^T + T[bucket, h]     P = softmax(S, rows)     out = P V     lse = logsumexp(S, rows)

``bfs_buckets`` is a breadth-first search per source node over out-neighbour lists; ``forward`` a dense attention per
graph and head with the bias gathered from the table.  ``table_terms`` gives, in float64, what the table's gradient is
a sum of: g_table[b, h] = sum over the pairs of bucket b of ds_ij, ds_ij = p_ij (<g_out_i, v_j> - delta_i) -- the sum
of |ds_ij|, the number of pairs per bucket and the single largest term (the toothed variant removes it).
``BiasedAttentionRef`` puts the bias into the attention of tests/gps_oracle.py's layer and model."""
import torch
import torch.nn as nn

from tests import gps_oracle as GPSO


def _graphs(ptr):
    p = [int(v) for v in ptr]
    return [(g, p[g], p[g + 1]) for g in range(len(p) - 1)]


def bfs_buckets(edge_index, ptr, max_dist, eptr=None):
    """A list with graph g's [n_g, n_g] uint8 bucket matrix (row = source / query, column = target / key).  Edges with
    an end outside their graph are left out (``eptr`` says which columns of ``edge_index`` belong to which graph; without
    it an edge belongs to the graph of its source)."""
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    out = []
    for g, s, e in _graphs(ptr):
        n = e - s
        succ = [[] for _ in range(n)]
        cols = range(len(src)) if eptr is None else range(int(eptr[g]), int(eptr[g + 1]))
        for c in cols:
            a, b = src[c] - s, dst[c] - s
            if eptr is None and not 0 <= a < n:
                continue
            if 0 <= a < n and 0 <= b < n:
                succ[a].append(b)
        M = torch.full((n, n), max_dist, dtype=torch.uint8)
        for i in range(n):
            dist = {i: 0}
            frontier = [i]
            d = 0
            while frontier and d + 1 < max_dist:
                d += 1
                nxt = []
                for u in frontier:
                    for v in succ[u]:
                        if v not in dist:
                            dist[v] = d
                            nxt.append(v)
                frontier = nxt
            for j, d in dist.items():
                if d < max_dist:
                    M[i, j] = d
        out.append(M)
    return out


def random_symmetric(n, seed, degree=3):
    """[2, E] int64: about ``degree`` n / 2 random undirected edges (both directions), no self-loops; n < 2: no edges."""
    if n < 2:
        return torch.zeros(2, 0, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(0, n, (2, max(1, degree * n // 2)), generator=g)
    e = e[:, e[0] != e[1]]
    return torch.cat([e, e.flip(0)], 1)


def edge_case_graphs():
    """(n, edge_index) per graph, local node ids: one node; no edges; two disconnected components; a directed 3-cycle
    (d(i, j) != d(j, i)); a path of 12 nodes (crosses a cap of 5); self-loops and duplicate edges; random symmetric
    graphs of n = 31, 32, 33, 63, 64, 65, 97 (the bitset word, the chunk and the tile edges)."""
    E = lambda pairs: torch.tensor(pairs, dtype=torch.int64).t().reshape(2, -1)
    both = lambda pairs: E(pairs + [(b, a) for a, b in pairs])
    graphs = [(1, E([])), (5, E([])),
              (7, both([(0, 1), (1, 2), (2, 3), (4, 5), (5, 6)])),
              (3, E([(0, 1), (1, 2), (2, 0)])),
              (12, both([(i, i + 1) for i in range(11)])),
              (6, E([(0, 0), (0, 1), (0, 1), (1, 2), (2, 2), (2, 3), (2, 3), (2, 3), (3, 4), (4, 4), (1, 0)]))]
    for n in (31, 32, 33, 63, 64, 65, 97):
        graphs.append((n, random_symmetric(n, 1000 + n)))
    return graphs


def collate(graphs):
    """(edge_index [2, E] with node offsets, ptr [B + 1] int64, eptr [B + 1] int64) of a list of (n, edge_index)."""
    ptr, eptr, parts = [0], [0], []
    for n, ei in graphs:
        parts.append(ei + ptr[-1])
        ptr.append(ptr[-1] + n)
        eptr.append(eptr[-1] + ei.size(1))
    return (torch.cat(parts, 1).contiguous(), torch.tensor(ptr, dtype=torch.int64),
            torch.tensor(eptr, dtype=torch.int64))


def flat(buckets):
    """(bucket [sum n^2] uint8, spd_ptr [B + 1] int64): the operator's layout of a list of matrices."""
    sizes = torch.tensor([m.numel() for m in buckets], dtype=torch.int64)
    sptr = torch.zeros(len(buckets) + 1, dtype=torch.int64)
    sptr[1:] = torch.cumsum(sizes, 0)
    data = torch.cat([m.reshape(-1) for m in buckets]) if buckets else torch.zeros(0, dtype=torch.uint8)
    return data, sptr


def forward(qkv, table, buckets, ptr, heads, skip=None, on_bias=None):
    """(out [N, D], lse [N, heads]) in qkv's dtype; differentiable in qkv and table.  ``skip = (g, j)`` leaves key j of
    graph g out (tests/attention_oracle.py's toothed variant).  ``on_bias(bias [n, keys, heads], bucket [n, keys])`` sees
    every graph's gathered bias (the table's gradient is the sum of that tensor's cotangent per bucket)."""
    N, D = qkv.size(0), qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    Q, K, V = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    outs, lses = [], []
    for g, s, e in _graphs(ptr):
        if e == s:
            continue
        keys = torch.arange(e - s)
        if skip is not None and skip[0] == g:
            keys = keys[keys != skip[1]]
        bias = table[buckets[g].long()[:, keys]]                  # [n, keys, heads]
        if on_bias is not None:
            on_bias(bias, buckets[g].long()[:, keys])
        o_g, l_g = [], []
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            S = (Q[s:e, c] @ K[s:e, c][keys].t()) * scale + bias[:, :, h]
            l_g.append(torch.logsumexp(S, 1))
            o_g.append(torch.softmax(S, 1) @ V[s:e, c][keys])
        outs.append(torch.cat(o_g, 1))
        lses.append(torch.stack(l_g, 1))
    if not outs:
        return qkv.new_zeros(0, D), qkv.new_zeros(0, heads)
    return torch.cat(outs), torch.cat(lses)


def run(qkv, table, buckets, ptr, heads, g_out, dtype):
    """{"out", "gQ", "gK", "gV", "g_table"} of ``forward`` in ``dtype`` through torch's autograd."""
    x = qkv.detach().clone().to(dtype).requires_grad_(True)
    t = table.detach().clone().to(dtype).requires_grad_(True)
    out, _ = forward(x, t, buckets, ptr, heads)
    out.backward(g_out.to(dtype))
    D = qkv.size(1) // 3
    return {"out": out.detach(), "gQ": x.grad[:, :D].clone(), "gK": x.grad[:, D:2 * D].clone(),
            "gV": x.grad[:, 2 * D:].clone(), "g_table": t.grad.detach().clone()}


def table_terms(qkv, table, buckets, ptr, heads, g_out):
    """In float64: ``mag`` [nb, heads] = the sum of |ds_ij| per bucket and head, ``count`` [nb] = the number of pairs per
    bucket, ``g_table`` [nb, heads] = the sum of ds_ij (the formula, not autograd), and ``largest`` = (value, b, h): the
    single largest |ds_ij| with its signed value and where it lands."""
    qkv, table, g_out = qkv.double(), table.double(), g_out.double()
    D = qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    nb = table.size(0)
    mag = torch.zeros(nb, heads, dtype=torch.float64)
    gt = torch.zeros(nb, heads, dtype=torch.float64)
    count = torch.zeros(nb, dtype=torch.int64)
    best = (0.0, 0, 0)
    for g, s, e in _graphs(ptr):
        if e == s:
            continue
        bk = buckets[g].long()
        count += torch.bincount(bk.reshape(-1), minlength=nb)
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            q, k, v = qkv[s:e, :D][:, c], qkv[s:e, D:2 * D][:, c], qkv[s:e, 2 * D:][:, c]
            P = torch.softmax((q @ k.t()) * scale + table[bk][:, :, h], 1)
            dP = g_out[s:e, c] @ v.t()
            dS = P * (dP - (P * dP).sum(1, keepdim=True))
            mag[:, h] += torch.zeros(nb, dtype=torch.float64).index_add_(0, bk.reshape(-1), dS.abs().reshape(-1))
            gt[:, h] += torch.zeros(nb, dtype=torch.float64).index_add_(0, bk.reshape(-1), dS.reshape(-1))
            idx = int(dS.abs().argmax())
            val = float(dS.reshape(-1)[idx])
            if abs(val) > abs(best[0]):
                best = (val, int(bk.reshape(-1)[idx]), h)
    return mag, count, gt, best


class _Table(nn.Module):
    def __init__(self, K, heads):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(K, heads).normal_(0.0, 0.5))


class BiasedAttentionRef(GPSO.AttentionRef):
    """tests/gps_oracle.py's ``AttentionRef`` with the table ``spd_bias.weight`` [K, heads] (the product's key) and the
    batch's bucket matrices in ``buckets`` (set before the call; not a parameter)."""

    def __init__(self, D, heads, K):
        super().__init__(D, heads)
        self.spd_bias = _Table(K, heads)
        self.buckets = None
        self.bias_hook = None                  # optional callable(bias, bucket) per graph (the tests' term magnitudes)

    def forward(self, x, ptr, skip=None):
        qkv = x @ self.in_proj_weight.t() + self.in_proj_bias
        if self.term_hook is not None:
            self.term_hook(qkv)
        return self.out_proj(forward(qkv, self.spd_bias.weight, self.buckets, ptr, self.heads, skip=skip,
                                     on_bias=self.bias_hook)[0])


def with_spd(ref, K, buckets):
    """``ref`` (a ``GPSLayerRef`` or ``GPSRef``) with every attention replaced by a ``BiasedAttentionRef`` of ``K``
    buckets that keeps the replaced module's projection weights; the tables are drawn from the global generator."""
    layers = ref.layers if hasattr(ref, "layers") else [ref]
    for layer in layers:
        old = layer.attn
        new = BiasedAttentionRef(old.in_proj_weight.size(1), old.heads, K)
        new.load_state_dict(old.state_dict(), strict=False)
        new.buckets = buckets
        layer.attn = new
    return ref
