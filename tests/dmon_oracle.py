"""Plain-torch restatement of DMoN pooling (Tsitsulin et al., "Graph Clustering with Graph Neural Networks"; PyG
``dense_dmon_pool``) as ``nn.pool.dmon_pool_sparse`` defines it, per graph on a dense adjacency built from the edge
list with multiplicities, in float32 or float64:

    A[r, c] += 1 per edge (r, c);  d_i = sum_c A[i, c];  2m = sum_i d_i;  S = softmax(logits)
    spectral = -( sum_i S_i . (A S)_i - sum_k (d^T S)_k^2 / 2m ) / 2m          (0 when 2m = 0)
    ortho    = | S^T S / |S^T S|_F - I / sqrt(K) |_F
    cluster  = | sum_i S_i |_2 sqrt(K) / n - 1
    pooled_x = selu(S^T X);  pooled_adj = S^T A S, diagonal zeroed, divided by sqrt(rowsum) + 1e-15 on both sides

every loss the mean over the graphs.  ``backward`` is the hand-written gradient of w_s spectral + w_o ortho +
w_c cluster with respect to the logits.  ``null`` / ``at_half`` / ``cluster`` = False leave one term out (the
null-model term, the A^T half of the spectral gradient, the cluster term): what the GPU test's bar must reject.
Also the seeded inputs shared by tests/test_dmon_host.py and tests/test_gpu_dmon.py."""
import math

import torch

SIZES = [1, 2, 37, 100, 130]
WEIGHTS = (1.3, 0.7, 0.9)


def graph_edges(n, g):
    """One graph's edge list [2, E] (local ids): random undirected edges, a self loop on every node and, beyond 3
    nodes, one duplicated edge and one edge present in one direction only."""
    loops = torch.arange(n).repeat(2, 1)
    if n == 1:
        return loops
    if n == 2:
        return torch.cat([torch.tensor([[0, 1], [1, 0]]), loops], 1)
    e = max(n, 3 * n // 2)
    src = torch.randint(0, n, (e,), generator=g)
    dst = (src + 1 + torch.randint(0, n - 1, (e,), generator=g)) % n        # never a loop
    und = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    parts = [und, loops]
    if n > 3:
        parts.append(und[:, :1])                                            # a duplicate
        parts.append(torch.tensor([[0], [n - 1]]))                          # 0 -> n-1 only (a third copy if present)
    return torch.cat(parts, 1)


def case(K, Fx, sizes=SIZES, seed=None):
    """(graphs = [(logits_g, x_g, edge_index_g)] in local ids) for the operator tests: logits N(0, 2^2)."""
    g = torch.Generator().manual_seed(1000 + 7 * K + Fx if seed is None else seed)
    out = []
    for n in sizes:
        ei = graph_edges(n, g)
        out.append((torch.randn(n, K, generator=g) * 2, torch.randn(n, Fx, generator=g), ei))
    return out


def flat(graphs):
    """(logits [N,K], x [N,Fx] or None, edge_index [2,E] in batch ids, sizes)."""
    sizes = [lg.size(0) for lg, _, _ in graphs]
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    logits = torch.cat([lg for lg, _, _ in graphs], 0)
    x = torch.cat([x for _, x, _ in graphs], 0)
    ei = torch.cat([e + o for (_, _, e), o in zip(graphs, offs)], 1)
    return logits, (x if x.size(1) else None), ei, sizes


def relabelled(graphs, seed):
    """``helpers.relabel_graphs`` applied to (logits | x | node id) rows: the relabelled graphs and, per graph, the old
    id of every new node (to carry node-indexed results back)."""
    from tests.helpers import relabel_graphs
    packed = [(torch.cat([lg, x, torch.arange(lg.size(0), dtype=lg.dtype).unsqueeze(1)], 1), ei) for lg, x, ei in graphs]
    out, olds = [], []
    for (lg, x, _), (p, ei) in zip(graphs, relabel_graphs(packed, seed)):
        K, Fx = lg.size(1), x.size(1)
        out.append((p[:, :K].contiguous(), p[:, K:K + Fx].contiguous(), ei))
        olds.append(p[:, -1].long())
    return out, olds


def dense_adj(ei, n, dtype, drop=None):
    A = torch.zeros(n, n, dtype=dtype)
    if drop is not None:
        keep = torch.ones(ei.size(1), dtype=torch.bool)
        keep[drop] = False
        ei = ei[:, keep]
    A.index_put_((ei[0], ei[1]), torch.ones(ei.size(1), dtype=dtype), accumulate=True)
    return A


def _ortho(ss, K):
    nrm = ss.norm()
    return (ss / nrm - torch.eye(K, dtype=ss.dtype) / math.sqrt(K)).norm(), nrm


def forward(graphs, dtype=torch.float64, null=True, cluster=True, drop_edge=None):
    """dict: S [N,K]; spectral / ortho / cluster (means, 0-dim); per graph [G]: trace, two_m, null, ss_norm, ortho_g,
    c_norm; ss [G,K,K]; vec [G,2,K]; pooled_x / pooled_adj (lists per graph).  ``drop_edge`` = (graph, edge) leaves one
    edge out of that graph's adjacency."""
    rows = {k: [] for k in ("trace", "two_m", "null", "ss_norm", "ortho_g", "c_norm", "spectral_g", "cluster_g")}
    Ss, sss, vecs, pxs, padjs = [], [], [], [], []
    for gi, (lg, x, ei) in enumerate(graphs):
        n, K = lg.shape
        A = dense_adj(ei, n, dtype, drop_edge[1] if drop_edge is not None and drop_edge[0] == gi else None)
        S = torch.softmax(lg.to(dtype), 1)
        d = A.sum(1)
        two_m = d.sum()
        AS = A @ S
        oa = S.t() @ AS
        trace = (S * AS).sum()
        dS = d @ S
        nullv = (dS * dS).sum() / two_m if float(two_m) > 0 and null else torch.zeros((), dtype=dtype)
        spectral = -(trace - nullv) / two_m if float(two_m) > 0 else torch.zeros((), dtype=dtype)
        ss = S.t() @ S
        o, nrm = _ortho(ss, K)
        c = S.sum(0)
        cl = c.norm() * math.sqrt(K) / n - 1 if cluster else torch.zeros((), dtype=dtype)
        for k, v in zip(rows, (trace, two_m, nullv, nrm, o, c.norm(), spectral, cl)):
            rows[k].append(v)
        Ss.append(S)
        sss.append(ss)
        vecs.append(torch.stack([dS, c]))
        pxs.append(torch.nn.functional.selu(S.t() @ x.to(dtype)))
        off = oa - torch.diag(torch.diag(oa))
        dn = off.sum(1).sqrt() + 1e-15
        padjs.append(off / dn.unsqueeze(0) / dn.unsqueeze(1))
    out = {k: torch.stack(v) for k, v in rows.items()}
    out.update(S=torch.cat(Ss, 0), ss=torch.stack(sss), vec=torch.stack(vecs), pooled_x=pxs, pooled_adj=padjs,
               spectral=out["spectral_g"].mean(), ortho=out["ortho_g"].mean(), cluster=out["cluster_g"].mean())
    return out


def backward(graphs, weights=WEIGHTS, dtype=torch.float64, null=True, at_half=True, cluster=True):
    """Hand-written d(w_s spectral + w_o ortho + w_c cluster)/d logits [N,K] (the issue's formulas)."""
    G = len(graphs)
    ws, wo, wc = (w / G for w in weights)
    outs = []
    for lg, _, ei in graphs:
        n, K = lg.shape
        A = dense_adj(ei, n, dtype)
        S = torch.softmax(lg.to(dtype), 1)
        d = A.sum(1)
        two_m = d.sum()
        dS = torch.zeros_like(S)
        if float(two_m) > 0:
            both = A @ S + (A.t() @ S if at_half else 0)
            nullg = 2 * d.unsqueeze(1) * (d @ S).unsqueeze(0) / two_m if null else 0
            dS = dS + ws * (-(both - nullg) / two_m)
        ss = S.t() @ S
        o, nrm = _ortho(ss, K)
        if float(o) > 0:
            Gq = (ss / nrm - torch.eye(K, dtype=dtype) / math.sqrt(K)) / o
            Gss = (Gq - (Gq * ss).sum() / (nrm * nrm) * ss) / nrm
            dS = dS + wo * (S @ (Gss + Gss.t()))
        if cluster:
            c = S.sum(0)
            dS = dS + wc * (math.sqrt(K) / n) * (c / c.norm()).unsqueeze(0)
        outs.append(S * (dS - (dS * S).sum(1, keepdim=True)))
    return torch.cat(outs, 0)


def autograd_backward(graphs, weights=WEIGHTS, dtype=torch.float64):
    """The same gradient by autograd through ``forward``."""
    leaves = [lg.to(dtype).clone().requires_grad_() for lg, _, _ in graphs]
    f = forward([(l, x, ei) for l, (_, x, ei) in zip(leaves, graphs)], dtype)
    (weights[0] * f["spectral"] + weights[1] * f["ortho"] + weights[2] * f["cluster"]).backward()
    return torch.cat([l.grad for l in leaves], 0)


def scalars(f):
    """The tensors of a forward the referee compares, as a dict: the three losses and the spectral loss's two
    terms per graph (trace / 2m and null / 2m: they cancel in the loss, so each is refereed at its own scale)."""
    tm = torch.where(f["two_m"] > 0, f["two_m"], torch.ones_like(f["two_m"]))
    return {"spectral": f["spectral"].reshape(1), "ortho": f["ortho"].reshape(1), "cluster": f["cluster"].reshape(1),
            "trace/2m": f["trace"] / tm, "null/2m": f["null"] / tm}


def draws32(graphs, n_draws=8, first_seed=1):
    """``n_draws`` float32 evaluations on relabelled copies: [{scalars..., "g_logits" carried back to the given node
    order}]."""
    out = []
    for s in range(first_seed, first_seed + n_draws):
        rg, olds = relabelled(graphs, s)
        d = scalars(forward(rg, torch.float32))
        g = backward(rg, dtype=torch.float32)
        back, off = torch.empty_like(g), 0
        for old in olds:
            back[off + old] = g[off:off + old.numel()]
            off += old.numel()
        d["g_logits"] = back
        out.append(d)
    return out


def referee_scaled(got, o32, o64, scale, what=""):
    """``helpers.referee``'s bar with the ulp term taken at ``scale`` instead of max|o64|: for the spectral loss, a
    difference of two terms of nearly equal size, the rounding of either term is what a float32 evaluation carries, so
    the scale is the larger term's magnitude.  |got - f64| / (2 max_r |o32_r - f64| + 8 * 2^-23 * scale)."""
    got, o64 = got.detach().cpu().double(), o64.detach().cpu().double()
    e_hip = float((got - o64).abs().max())
    e_o32 = max(float((t.detach().cpu().double() - o64).abs().max()) for t in o32)
    lim = 2.0 * e_o32 + 8.0 * 2.0 ** -23 * float(scale)
    ratio = e_hip / lim if lim > 0.0 else (0.0 if e_hip == 0.0 else float("inf"))
    if not ratio == ratio:
        ratio = float("inf")
    print(f"   referee {what:56s} |got-f64| = {e_hip:.3e}  |oracle32-f64| = {e_o32:.3e}  scale = {float(scale):.3e}  "
          f"ratio = {ratio:.3f}")
    return ratio


def referee_case(got, graphs, what=""):
    """The operator's bar: ``got`` = {spectral, ortho, cluster [1]; trace/2m, null/2m [G]; g_logits [N,K]} (``scalars``
    of a forward plus the gradient of WEIGHTS . losses) against the float64 oracle, the yardstick eight relabelled
    float32 oracle draws; then the bar's teeth: it must reject the float64 oracle with the null-model term, the A^T half
    of the gradient or the cluster term left out.  At K = 1 the gradient and the cluster loss vanish identically, with
    or without any term, so only the null-model term's absence is visible there (in the loss).  Returns the worst
    ratio of the true comparison."""
    from tests.helpers import referee, teeth
    K = graphs[0][0].size(1)
    f64 = forward(graphs)
    o64 = dict(scalars(f64), g_logits=backward(graphs))
    o32 = draws32(graphs)
    sp_scale = max(abs(float(o64["trace/2m"].mean())), abs(float(o64["null/2m"].mean())))
    worst = referee_scaled(got["spectral"], [d["spectral"] for d in o32], o64["spectral"], sp_scale, f"{what} spectral")
    assert worst <= 1.0, f"{what} spectral: outside the float64 referee (ratio {worst:.3f})"
    for k in ("ortho", "cluster", "trace/2m", "null/2m", "g_logits"):
        r = referee(got[k], [d[k] for d in o32], o64[k], f"{what} {k}")
        assert r <= 1.0, f"{what} {k}: outside the float64 referee (ratio {r:.3f})"
        worst = max(worst, r)
    # teeth: the null-model term
    no_null = forward(graphs, null=False)
    shifted = [d["spectral"].double() - o64["spectral"] + no_null["spectral"].reshape(1) for d in o32]
    r = referee_scaled(got["spectral"], shifted, no_null["spectral"].reshape(1), sp_scale, f"{what} spectral [no null model]")
    assert r > 1.0, f"{what}: the bar cannot see a missing null-model term in the loss (ratio {r:.3f})"
    dropped = {"null/2m": scalars(no_null)["null/2m"]}
    if K > 1:
        dropped["g_logits"] = backward(graphs, null=False)
    teeth(got, o32, o64, dropped, f"{what} [no null model]")
    if K > 1:
        teeth(got, o32, o64, {"g_logits": backward(graphs, at_half=False)}, f"{what} [no A^T half]")
        teeth(got, o32, o64, {"g_logits": backward(graphs, cluster=False),
                              "cluster": forward(graphs, cluster=False)["cluster"].reshape(1)}, f"{what} [no cluster term]")
    return worst
