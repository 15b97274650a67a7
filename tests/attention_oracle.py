"""Plain-torch restatement of block-diagonal multi-head self-attention, written from the formula (CPU, float32 or
float64): for every graph g = rows [ptr[g], ptr[g + 1]) and head h (columns [h dh, (h + 1) dh) of each third of qkv)

    S = scale Q K^T      P = softmax(S, rows)      out = P V      lse = logsumexp(S, rows)      scale = dh^-1/2

``forward`` loops over graphs and heads; ``skip=(g, j)`` leaves key j of graph g out (the toothed variant);
``boundary=+1`` lets the first key of the next graph in and ``interleaved=True`` takes head h from columns h, h + heads,
... (the two wrong layouts the tests must reject).  ``backward`` is the hand-written gradient (``no_delta=True`` omits
the softmax's -delta_i term); ``magnitudes`` the quantities of the a-priori bound."""
import torch


def _graphs(ptr):
    p = [int(v) for v in ptr]
    return [(g, p[g], p[g + 1]) for g in range(len(p) - 1)]


def _cols(h, dh, heads, interleaved):
    if interleaved:
        return torch.arange(dh) * heads + h
    return torch.arange(h * dh, (h + 1) * dh)


def forward(qkv, ptr, heads, skip=None, boundary=0, interleaved=False):
    """(out [N, D], lse [N, heads]) in qkv's dtype; differentiable."""
    N, D = qkv.size(0), qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    Q, K, V = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    outs, lses = [], []
    for g, s, e in _graphs(ptr):
        if e == s:
            continue
        ke = min(e + boundary, N) if boundary > 0 else e
        keys = torch.arange(s, ke)
        if skip is not None and skip[0] == g:
            keys = keys[keys != s + skip[1]]
        o_g, l_g = [], []
        for h in range(heads):
            c = _cols(h, dh, heads, interleaved)
            S = (Q[s:e][:, c] @ K[keys][:, c].t()) * scale
            l_g.append(torch.logsumexp(S, 1))
            o_g.append((torch.softmax(S, 1) @ V[keys][:, c], c))
        og = qkv.new_zeros(e - s, D)
        cols = torch.cat([c for _, c in o_g])
        og = og.index_copy(1, cols, torch.cat([o for o, _ in o_g], 1))
        outs.append(og)
        lses.append(torch.stack(l_g, 1))
    if not outs:
        return qkv.new_zeros(0, D), qkv.new_zeros(0, heads)
    return torch.cat(outs), torch.cat(lses)


def backward(qkv, ptr, heads, g_out, no_delta=False):
    """g_qkv [N, 3D] by the formulas of the two backward passes (not autograd)."""
    N, D = qkv.size(0), qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    g = torch.zeros_like(qkv)
    for _, s, e in _graphs(ptr):
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            q, k, v = qkv[s:e, :D][:, c], qkv[s:e, D:2 * D][:, c], qkv[s:e, 2 * D:][:, c]
            go = g_out[s:e, c]
            P = torch.softmax((q @ k.t()) * scale, 1)
            dP = go @ v.t()
            delta = torch.zeros(e - s, 1, dtype=qkv.dtype) if no_delta else (P * dP).sum(1, keepdim=True)
            dS = P * (dP - delta)
            g[s:e, c] = scale * (dS @ k)
            g[s:e, D + h * dh:D + (h + 1) * dh] = scale * (dS.t() @ q)
            g[s:e, 2 * D + h * dh:2 * D + (h + 1) * dh] = P.t() @ go
    return g


def autograd_backward(qkv, ptr, heads, g_out, dtype, skip=None):
    """(out, g_qkv) of ``forward`` in ``dtype`` through torch's autograd."""
    x = qkv.detach().clone().to(dtype).requires_grad_(True)
    out, _ = forward(x, ptr, heads, skip=skip)
    out.backward(g_out.to(dtype))
    return out.detach(), x.grad.detach()


def magnitudes(qkv, ptr, heads):
    """``a`` [N, heads]: max_j scale sum_d |q_id| |k_jd| of the row; ``mag`` [N, D]: sum_j p_ij |v_jd|; ``n`` [N, 1]:
    the row's number of keys.  All in float64."""
    qkv = qkv.double()
    N, D = qkv.size(0), qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    a = torch.zeros(N, heads, dtype=torch.float64)
    mag = torch.zeros(N, D, dtype=torch.float64)
    n = torch.zeros(N, 1, dtype=torch.float64)
    for _, s, e in _graphs(ptr):
        n[s:e] = e - s
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            q, k, v = qkv[s:e, :D][:, c], qkv[s:e, D:2 * D][:, c], qkv[s:e, 2 * D:][:, c]
            if e > s:
                a[s:e, h] = ((q.abs() @ k.abs().t()) * scale).max(1).values
                mag[s:e, c] = torch.softmax((q @ k.t()) * scale, 1) @ v.abs()
    return a, mag, n


def largest_message(qkv, ptr, heads):
    """(g, j, i, h): the single largest |p_ij v_j| (max over the head's columns) among graphs of more than one node."""
    qkv = qkv.double()
    D = qkv.size(1) // 3
    dh = D // heads
    scale = dh ** -0.5
    best = (-1.0, None)
    for g, s, e in _graphs(ptr):
        if e - s < 2:
            continue
        for h in range(heads):
            c = slice(h * dh, (h + 1) * dh)
            q, k, v = qkv[s:e, :D][:, c], qkv[s:e, D:2 * D][:, c], qkv[s:e, 2 * D:][:, c]
            M = torch.softmax((q @ k.t()) * scale, 1) * v.abs().max(1).values.unsqueeze(0)
            val, idx = M.flatten().max(0)
            if float(val) > best[0]:
                i, j = divmod(int(idx), e - s)
                best = (float(val), (g, j, i, h))
    return best[1]


def drop_message(out64, qkv, ptr, heads, where):
    """``out64`` with the message p_ij v_j of ``where = (g, j, i, h)`` removed from row i (p of the FULL softmax)."""
    g, j, i, h = where
    qkv = qkv.double()
    D = qkv.size(1) // 3
    dh = D // heads
    s, e = int(ptr[g]), int(ptr[g + 1])
    c = slice(h * dh, (h + 1) * dh)
    q, k, v = qkv[s:e, :D][:, c], qkv[s:e, D:2 * D][:, c], qkv[s:e, 2 * D:][:, c]
    P = torch.softmax((q @ k.t()) * dh ** -0.5, 1)
    out = out64.clone()
    out[s + i, c] -= P[i, j] * v[j]
    return out
