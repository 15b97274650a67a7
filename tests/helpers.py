"""Shared builders for the parity tests (seeded inputs, oracle <-> product weights)."""
import numpy as np
import torch

from graph_hscn.loader.synthetic import make_dataset
from oracle import hetero_data as OH

DEV = "cuda"
ATOL = 1e-5      # north_star: float activations within 1e-5 of the CPU path
RTOL = 1e-5


def rand_graph(n, e, seed, symmetric=False, self_loops=False):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    if not self_loops:
        keep = src != dst
        src, dst = src[keep], dst[keep]
    ei = torch.stack([src, dst])
    if symmetric:
        ei = torch.cat([ei, ei.flip(0)], 1)
    return ei


def hetero_batch(name, num_graphs, K, seed):
    graphs = make_dataset(name, num_graphs, seed=seed)
    rng = np.random.default_rng(seed)
    hs = [OH.hetero_from_clusters(g.x, g.edge_index, g.y, rng.integers(0, K, g.num_nodes), K) for g in graphs]
    return OH.collate_hetero(hs), graphs


def close(a, b, atol=ATOL, rtol=RTOL):
    a = a.detach().cpu()
    b = b.detach().cpu()
    ok = torch.allclose(a, b, atol=atol, rtol=rtol)
    if not ok:
        d = (a - b).abs()
        print("max abs diff", float(d.max()), "at", int(d.argmax()), "ref", float(b.flatten()[d.argmax()]))
    return ok


def scale_close(a, b, rel=1e-5):
    """max|a - b| <= rel * max(1, max|b|): the 1e-5 bar read relative to the magnitude of the tensor.  Used for
    outputs whose elements are sums of terms of size ~max|b| that cancel (the virtual-node features: a ReLU of
    GAT + GCN rows whose terms reach 10^1..10^2 on integer atom features) -- there an absolute 1e-5 on an element
    near zero asks for more than float32 holds (2^-23 * 67 = 8e-6 per rounding).  That HIP is no further from
    the float64 value than the float32 oracle is shown separately
    (tests/test_gpu_resident.py::test_hip_is_as_close_to_float64_as_the_float32_oracle)."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    d = float((a - b).abs().max()) if a.numel() else 0.0
    lim = rel * max(1.0, float(b.abs().max()) if b.numel() else 0.0)
    if d > lim:
        print("max abs diff", d, "limit", lim)
    return d <= lim


def grads_close(a, b, rel=2e-6):
    """Two float32 evaluations of the same gradient that group their partial sums differently (the one-launch step
    sums a weight gradient per 16-row tile, the launch pair per strided row chunk): equal to a few ulp of the
    gradient's magnitude."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    lim = rel * max(1e-6, float(b.abs().max()))
    d = float((a - b).abs().max()) if a.numel() else 0.0
    if d > lim:
        print("max abs diff", d, "limit", lim)
    return d <= lim


def pool_order_close(a, b, rel=1e-5):
    """Outputs of the one-launch step's head against the launch pair's: the same head applied to a mean pool whose
    partial sums are grouped differently -- per wave out of the last layer's accumulators (rows of a tile, tiles of a
    wave, waves) instead of a strided pass over the finished layer.  n <= 444 non-negative (post-ReLU) terms: either
    grouping is within (n - 1) 2^-24 <= 2.7e-5 of the exact sum in the worst case and ~sqrt(n) 2^-24 ~ 1e-6 typically;
    the bar applied is north_star's 1e-5, relative to the tensor's magnitude.  Returns the verdict; prints the distance
    when it fails."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    d = float((a - b).abs().max()) if a.numel() else 0.0
    lim = rel * max(1.0, float(b.abs().max()) if b.numel() else 0.0)
    if d > lim:
        print("pool-order distance", d, "limit", lim)
    return d <= lim


U32 = 2.0 ** -24     # unit roundoff of float32 (round to nearest)
F64_C = 3.0          # the one constant of the a-priori bound below; never tuned per test


def f64_close(got, ref, mag, n, c=F64_C, tiny=1e-30, what=""):
    """A float32 kernel result against the same operation evaluated in float64 on the same float32 inputs, element by
    element:  |got - ref| <= c * n * 2^-24 * mag + tiny.

    Linear operations (sums of products: linear, spmm, segment sums, weight gradients, pooled products): ``ref`` is
    the float64 value and ``mag`` the same operation evaluated in float64 on absolute values (|x| |W|^T + |b|,
    sum |w| |h|, ...); ``n`` is the length of the sum behind the element (scalar or broadcastable tensor), counting the
    bias / accumulate / epilogue additions.  Any order of float32 fma / mul+add evaluation is within
    n * 2^-24 * sum|terms| of the exact sum to first order (Higham, Accuracy and Stability, eq. 3.5, with gamma_n ~
    n u), and so is an ordered tree of chunk partials.  c = 3 covers the output rounding and the second-order terms.

    Non-linear operations: the bound is the linear one on their inputs propagated through the op's condition, folded
    into ``n`` and ``mag`` by the caller, so the form stays the same:
      * relu / elu / tanh (Lipschitz <= 1): the pre-activation bound plus a few ulp of |y| for the library function
        (mag gains |y|, n gains 4);
      * softmax-weighted sums (GAT): alpha_e = exp(z_e - m) / sum carries a relative error ~ u (|z_e| + |m|) from
        rounding the score and the shift before exp, plus ~deg u from the exp-sum: n = deg + 4 + max |z| + |m| with
        mag = sum alpha |h| + |b|;
      * normalisation (LayerNorm / BatchNorm): y = (x - mu) rstd: mu and var are sums of length N (or H); the error of
        the centred value is ~ n u (|x| + |mu|), scaled by rstd: mag = (|x| + |mu|) rstd |gamma| + |beta|.  A one-pass
        variance E[x^2] - mu^2 loses (mu/std)^2 u relative, far outside this for a column with mean 1e4, std 1;
      * MinCUT losses and the criterion: a ratio / mean of sums: n = the longest sum feeding it (+ a few), mag the
        same expression in absolute values or, where it has no sign structure, the float64 result's scale.

    Returns the verdict; prints the worst element when it fails."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    mag = torch.as_tensor(mag).detach().cpu().double()
    n = torch.as_tensor(n, dtype=torch.float64).detach().cpu()
    if got.shape != ref.shape:
        print(what, "shape", tuple(got.shape), "vs", tuple(ref.shape))
        return False
    if got.numel() == 0:
        return True
    lim = c * n * U32 * mag + tiny
    d = (got - ref).abs()
    bad = ~(d <= lim)
    if bool(bad.any()):
        excess = torch.where(bad, d / lim.expand_as(d), torch.zeros_like(d))
        k = int(torch.nan_to_num(excess, nan=float("inf")).argmax())
        print(what, "f64 bound violated at", k, "got", float(got.flatten()[k]), "ref", float(ref.flatten()[k]),
              "diff", float(d.flatten()[k]), "limit", float(lim.expand_as(d).flatten()[k]))
        return False
    return True


def check_f64(got, ref, mag, n, dropped, c=F64_C, tiny=1e-30, what=""):
    """``f64_close`` plus its teeth: ``dropped`` is a second float64 reference with the largest-magnitude single term
    of the sum removed (one edge, one row, one input column, one chunk).  The kernel result must pass against ``ref``
    and be REJECTED against ``dropped`` by the same bound -- a bar loose enough to accept a missing term proves
    nothing."""
    assert f64_close(got, ref, mag, n, c, tiny, what), f"{what}: outside the float64 bound"
    assert not f64_close(got, dropped, mag, n, c, tiny), f"{what}: the bound cannot see a dropped term"


def drop_largest_product(ref, a, b, post=None):
    """``ref`` ([R, O] = a [R, I] @ b [I, O] in float64, possibly through an element-wise ``post``) with the largest
    |a[r, i] b[i, o]| removed from its element.  Found without forming the [R, I, O] product: per i, the largest |a|
    of the column times the largest |b| of the row.  ``post(pre, r, o)`` recomputes the element from its
    pre-activation when an epilogue follows."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    out = ref.detach().cpu().double().clone()
    if post is not None and a.numel() * b.shape[1] <= 1 << 23:
        # an epilogue can hide a term (relu of an element that stays negative): the largest term whose removal
        # changes its element
        terms = a.unsqueeze(2) * b.unsqueeze(0)                            # [R, I, O]
        order = torch.argsort(terms.abs().flatten(), descending=True)
        R, I, O = terms.shape
        for k in order[:4096].tolist():
            r, rest = divmod(k, I * O)
            i, o = divmod(rest, O)
            v = post(r, o, float(terms[r, i, o]))
            if v != float(out[r, o]):
                out[r, o] = v
                return out
    ca, ra = a.abs().max(0)
    cb, ob = b.abs().max(1)
    i = int((ca * cb).argmax())
    r, o = int(ra[i]), int(ob[i])
    t = float(a[r, i] * b[i, o])
    out[r, o] = post(r, o, t) if post is not None else out[r, o] - t
    return out
