"""The LapPE node encoder's DeepSet model, restated in torch (float64 unless told otherwise): the project's definition
of GraphGPS's ``LapPENodeEncoder`` (include/hscn.h: hscn_lappe_fwd / hscn_lappe_bwd).

    u_ik = (s_k vec[i,k], val[i,k])                          NaN entries read as 0
    a^0 = relu(W_0 u + b_0),  a^l = relu(W_l a^{l-1} + b_l)
    pe_sum[i] = sum over the k with vec[i,k] not NaN of a^{L-1}_ik

``s_k`` = -1 iff flips are on and word 0 of philox4x32_10(seed, ctr = k) is >= 2^31 (``signs``, over the Philox
restatement of tests/test_gpu_exact_edges.py).  ``chain`` evaluates the definition with hand-written gradients for the
parameters (checked against autograd in tests/test_lappe_host.py) and, with ``absolute=True``, the same sums over
absolute values: the ``mag`` of ``helpers.f64_close``'s bound."""
import numpy as np
import torch


def signs(K, seed):
    """[K] float64 of +-1: the flips of a call under ``seed`` (None: no flips)."""
    if seed is None:
        return torch.ones(K, dtype=torch.float64)
    from tests.test_gpu_exact_edges import philox4x32_10
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((K, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(K, dtype=np.uint64)
    w0 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[:, 0].astype(np.uint64)
    return torch.from_numpy(np.where(w0 >= np.uint64(2 ** 31), -1.0, 1.0))


def widths(dim_pe, layers):
    return [2] + [2 * dim_pe] * (layers - 1) + [dim_pe]


def chain(vec, val, Ws, bs, sign=None, g=None, absolute=False, drop_freq=None, dtype=torch.float64):
    """``(pe_sum [N, dim_pe], grads or None, margin)``.  ``sign``: [K] of +-1 or None.  ``g`` [N, dim_pe]: the cotangent
    of ``pe_sum``; ``grads`` is then the list [gW_0, gb_0, gW_1, gb_1, ...].  ``drop_freq``: that frequency column is
    left out of the sum (the bound's tooth).  ``absolute``: every product and sum over absolute values, with the ReLU
    gates of the true evaluation (forward: all terms are non-negative, the gates are open).  ``margin``: the smallest
    |pre-activation| over the samples that count (how far the nearest ReLU gate is from flipping)."""
    vec, val = vec.detach().cpu().to(dtype), val.detach().cpu().to(dtype)
    Ws = [W.detach().cpu().to(dtype) for W in Ws]
    bs = [b.detach().cpu().to(dtype) for b in bs]
    N, K = vec.shape
    valid = ~torch.isnan(vec)
    if drop_freq is not None:
        valid = valid.clone()
        valid[:, drop_freq] = False
    s = torch.ones(K, dtype=dtype) if sign is None else sign.to(dtype)
    u = torch.stack((torch.nan_to_num(vec, nan=0.0) * s, torch.nan_to_num(val, nan=0.0)), 2)      # [N, K, 2]
    acts, gates, margin = [u], [], float("inf")
    a = u
    for W, b in zip(Ws, bs):                       # the true evaluation: values and gates
        z = a @ W.t() + b
        if bool(valid.any()):
            margin = min(margin, float(z[valid].abs().min()))
        gates.append(z > 0)
        a = torch.relu(z)
        acts.append(a)
    if absolute:
        acts, a = [u.abs()], u.abs()
        for W, b in zip(Ws, bs):
            a = a @ W.abs().t() + b.abs()
            acts.append(a)
    mask = valid.unsqueeze(2).to(dtype)
    pe = (acts[-1] * mask).sum(1)
    if g is None:
        return pe, None, margin
    g = g.detach().cpu().to(dtype)
    if absolute:
        g = g.abs()
    delta = g.unsqueeze(1) * mask * gates[-1].to(dtype)                                         # [N, K, H_{L-1}]
    grads = [None] * (2 * len(Ws))
    for l in range(len(Ws) - 1, -1, -1):
        d2, a2 = delta.reshape(N * K, -1), acts[l].reshape(N * K, -1)
        grads[2 * l], grads[2 * l + 1] = d2.t() @ a2, d2.sum(0)
        if l:
            W = Ws[l].abs() if absolute else Ws[l]
            delta = (delta @ W) * gates[l - 1].to(dtype)
    return pe, grads, margin


def bound_n(dim_pe, layers, K):
    """n of the a-priori bound for ``pe_sum``: per layer its fan-in, the bias and 4 for the ReLU, plus the K-term sum."""
    w = widths(dim_pe, layers)
    return sum(fan_in + 1 + 4 for fan_in in w[:-1]) + K


def make_inputs(N, K, dim_pe, layers, seed):
    """Seeded float32 inputs: ``vec`` / ``val`` [N, K] where row i (of at least 3 rows) has 1 + i % K valid
    frequencies -- graphs smaller than K -- and the rest NaN, row 1 (when there is one beyond row 0) is all NaN; Linear
    parameters drawn as the library's ``Linear`` draws them (uniform in +- 1 / sqrt(fan_in)); a cotangent ``g``."""
    gen = torch.Generator().manual_seed(seed)
    vec = torch.randn(N, K, generator=gen)
    val = torch.rand(N, K, generator=gen) * 2.0
    for i in range(N):
        keep = K if N < 3 else 1 + i % K
        vec[i, keep:] = float("nan")
        val[i, keep:] = float("nan")
    if N >= 3:
        vec[1], val[1] = float("nan"), float("nan")
    w = widths(dim_pe, layers)
    Ws, bs = [], []
    for i, o in zip(w[:-1], w[1:]):
        bound = 1.0 / i ** 0.5
        Ws.append((torch.rand(o, i, generator=gen) * 2 - 1) * bound)
        bs.append((torch.rand(o, generator=gen) * 2 - 1) * bound)
    g = torch.randn(N, dim_pe, generator=gen)
    return vec, val, Ws, bs, g
