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


# --------------------------------------------------------------------------- #
# float64 as the referee between two float32 evaluations (tests/test_gpu_layered_f64.py and the gradient checks of
# test_gpu_ops.py / test_gpu_models.py / test_gpu_mpnn.py; the bar of tests/test_gpu_full_size.py, constants unchanged)
# --------------------------------------------------------------------------- #
def referee(got, o32, o64, what=""):
    """One tensor in max norm:  |HIP - f64| <= 2 |oracle_f32 - f64| + 8 * 2^-23 * max|f64|.

    ``o32`` and ``o64`` are the CPU oracle's float32 and float64 evaluations of the same tensor from identical weights
    and inputs (``copy.deepcopy(om).double()``).  Both float32 results are sums of the same terms in different orders,
    each within the same a-priori bound of the exact value; the factor 2 covers that their rounding errors are
    independent draws, the 8 ulp of the tensor's scale a tensor whose float32 oracle happens to be exact.  Prints the
    three numbers and returns |HIP - f64| / limit (<= 1 passes; ``inf`` for a shape mismatch).

    ``o32`` may be a LIST of float32 oracle evaluations of the same tensor (the inputs as given and relabelled copies
    of them, ``relabel_graphs``: the same sum in exact arithmetic, another summation order each): the yardstick is then
    max_r |o32_r - f64|.  One evaluation's distance is one draw of a rounding error; for a sum that cancels (the MinCUT
    gradients) a single draw rejects a correct float32 evaluation about one time in ten.  A
    single tensor gives what it always gave, bit for bit."""
    got = got.detach().cpu().double()
    draws = [t.detach().cpu().double() for t in (o32 if isinstance(o32, (list, tuple)) else [o32])]
    o32 = draws[0]
    o64 = o64.detach().cpu().double()
    if got.shape != o64.shape or any(t.shape != o64.shape for t in draws):
        print(f"   referee {what}: shape {tuple(got.shape)} vs {tuple(o32.shape)} vs {tuple(o64.shape)}")
        return float("inf")
    if o64.numel() == 0:
        return 0.0
    e_hip = float((got - o64).abs().max())
    e_o32 = max(float((t - o64).abs().max()) for t in draws)
    ulp = 2.0 ** -23 * float(o64.abs().max())
    lim = 2.0 * e_o32 + 8.0 * ulp
    ratio = e_hip / lim if lim > 0.0 else (0.0 if e_hip == 0.0 else float("inf"))
    if not ratio == ratio:          # NaN anywhere fails
        ratio = float("inf")
    print(f"   referee {what:56s} |HIP-f64| = {e_hip:.3e}  |oracle32-f64| = {e_o32:.3e}  ulp(scale) = {ulp:.3e}  "
          f"ratio = {ratio:.3f}" + (f"  (max over {len(draws)} float32 draws)" if len(draws) > 1 else ""))
    return ratio


def _per_key(o32, k):
    """``o32``: a dict of tensors, or a list of such dicts (several float32 draws) -> what ``referee`` takes for ``k``."""
    return [d[k] for d in o32] if isinstance(o32, (list, tuple)) else o32[k]


def _shifted(o32, k, full, d):
    """The float32 draw(s) of tensor ``k`` carried over to the reference ``d``: their own distance to ``full`` kept."""
    if isinstance(o32, (list, tuple)):
        return [t[k].detach().cpu().double() - full + d for t in o32]
    return o32[k].detach().cpu().double() - full + d


def relabel_graphs(graphs, seed):
    """A relabelled copy of a list of ``(x, edge_index)`` graphs: per graph a node permutation applied to ``x`` and to
    the edge endpoints, then the edge order shuffled.  The same graphs -- any permutation-invariant function of them
    (the MinCUT losses, every parameter gradient) is equal in exact arithmetic -- with every sum over nodes or edges
    taken in another order: a float32 oracle evaluation of it is a further draw of the float32 rounding error."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for x, ei in graphs:
        n = x.size(0)
        perm = torch.randperm(n, generator=g)                   # new node j is old node perm[j]
        new_of_old = torch.empty(n, dtype=torch.long)
        new_of_old[perm] = torch.arange(n)
        e2 = new_of_old[ei] if ei.numel() else ei.clone()
        out.append((x[perm].contiguous(), e2[:, torch.randperm(ei.size(1), generator=g)].contiguous()))
    return out


def referee_all(got, o32, o64, what="", terms=None, cancelling=()):
    """``referee`` over dicts of tensors with the same keys (a key whose oracle value is None must be None in ``got``:
    the same gradient-less pattern on both sides).  Asserts every tensor; returns the worst ratio.  ``o32``: one dict,
    or a list of dicts (several float32 draws, see ``referee``).

    ``cancelling``: the tensors of THIS case, named explicitly by the caller with the reason, whose sum cancels so far
    that the referee's scale max|grad| says nothing about it.  Only these may, when the referee rejects them, pass by
    the a-priori bound of ``terms`` (the ``TermMagnitudes`` of the float64 run) instead; every other tensor passes the
    referee or the test fails.  Prints which tensors took the bound."""
    all32 = o32 if isinstance(o32, (list, tuple)) else [o32]
    for d in all32:
        assert set(d) == set(o64), (sorted(d), sorted(o64))
    assert set(got) == set(o64), (sorted(got), sorted(o64))
    assert set(cancelling) <= set(o64), sorted(set(cancelling) - set(o64))
    worst, derived = 0.0, []
    for k in o64:
        if o64[k] is None:
            assert all(d[k] is None for d in all32) and got[k] is None, \
                f"{what} {k}: the oracle leaves this gradient at None"
            continue
        assert got[k] is not None, f"{what} {k}: no gradient, the oracle has one"
        r = referee(got[k], _per_key(o32, k), o64[k], f"{what} {k}")
        if r > 1.0 and k in cancelling and terms is not None and terms.bound_holds(k, got[k], o64[k], what):
            derived.append((k, round(r, 3)))
            continue
        assert r <= 1.0, f"{what} {k}: outside the float64 referee (ratio {r:.3f})"
        worst = max(worst, r)
    print(f"   worst |HIP - f64| / (2 |oracle32 - f64| + 8 ulp) of {what}: {worst:.3f}"
          + (f"; held to the a-priori bound instead (referee ratio): {derived}" if derived else ""))
    return worst


def most_changed(full64, dropped64_list):
    """Per tensor of ``full64`` the candidate of ``dropped64_list`` (float64 gradient dicts with one term removed) that
    changes it most, for the tensors a removed term reaches at all (beyond float64 noise): {key: dropped tensor}."""
    best = {}
    for d in dropped64_list:
        for k, full in full64.items():
            if full is None or not full.numel():
                continue
            change = float((d[k] - full).abs().max())
            if change > best.get(k, (0.0, None))[0]:
                best[k] = (change, d[k])
    return {k: v[1] for k, v in best.items() if v[0] > 1e-12 * max(float(full64[k].abs().max()), 1e-300)}


def teeth(got, o32, o64, dropped64, what=""):
    """The referee's teeth (the mirror of ``check_f64``): ``dropped64`` is the float64 oracle with one term removed --
    for every tensor it checks, the HIP result must be REJECTED against it by the same ``referee`` (the float32 oracle's
    own distance stays the one to the TRUE float64 value: the bar is the same bar)."""
    for k in dropped64:
        if dropped64[k] is None:
            continue
        d = dropped64[k].detach().cpu().double()
        full = o64[k].detach().cpu().double()
        r = referee(got[k], _shifted(o32, k, full, d), d, f"{what} {k} [one term dropped]")
        assert r > 1.0, f"{what} {k}: the referee cannot see a dropped term (ratio {r:.3f})"


class KinkGuard:
    """Condition on the REFERENCE: a ReLU between layers and the GAT leaky-ReLU make a gradient discontinuous in the
    forward values.  Forward hooks on the float64 oracle record every ReLU input (``relu_after(module)``: the module's
    output feeds a ReLU) and every GAT attention logit (``attach`` finds the oracle's GATConv modules, which keep the
    logits of their last call); ``check(bar)`` asserts each is farther from zero than 4 x the forward bar the test
    asserts for that tensor, so that -- the forward check having passed -- no gate can differ between HIP, the float32
    oracle and float64.  An exact zero (a row no edge reaches under a zero bias) counts as a kink."""

    def __init__(self):
        self.values = []          # (tag, flat float64 tensor)
        self._handles = []

    def watch(self, tag, t):
        outs = t.values() if isinstance(t, dict) else [t]
        for o in outs:
            self.values.append((tag, o.detach().double().flatten()))
        return t

    def relu_after(self, module, tag="relu input"):
        self._handles.append(module.register_forward_hook(lambda m, a, out: (self.watch(tag, out), None)[1]))
        return self

    def attach(self, model):
        """Every oracle GATConv below ``model``: its attention logits (the leaky-ReLU's inputs)."""
        from oracle import pyg_ops as P
        for m in model.modules():
            if isinstance(m, P.GATConv):
                self._handles.append(m.register_forward_hook(
                    lambda mod, a, out: (self.watch("gat logit", mod.last_logits), None)[1]))
        return self

    def close(self):
        for h in self._handles:
            h.remove()
        self._handles = []

    def margin(self):
        return min([float(v.abs().min()) for _, v in self.values if v.numel()], default=float("inf"))

    def check(self, atol, rtol=0.0, what=""):
        """``atol`` / ``rtol``: the forward bar the test asserts, in ``close``'s element-wise form atol + rtol |v|."""
        worst = float("inf")
        for tag, v in self.values:
            if v.numel():
                r = v.abs() / (4.0 * (atol + rtol * v.abs()))
                k = int(r.argmin())
                worst = min(worst, float(r[k]))
                assert float(r[k]) > 1.0, (f"{what}: {tag} comes within {float(v[k].abs()):.3e} of its kink "
                                           f"(needs > 4 x {atol + rtol * float(v[k].abs()):.1e})")
        print(f"   kink guard {what}: smallest |gate input| = {self.margin():.3e} over {len(self.values)} tensors, "
              f"{worst:.1f} x the required distance")


class TermMagnitudes:
    """The a-priori form behind ``f64_close`` for a PARAMETER gradient whose sum cancels, recorded from the float64
    oracle while it runs.  Every parameter gradient is a sum over rows r (nodes, graphs) of cotangent row x input row:

        Linear      dW = sum_r g[r]^T x[r]          db = sum_r g[r]
        conv bias   db = sum_r g[r]                 (GCNConv / GATConv add it to the propagated rows)
        GAT att     d att_src = sum_r g_alpha_src[r] h_src[r]        (att_dst alike)
        norm layers d gamma = sum_r g[r] xhat[r]    d beta = sum_r g[r]

    ``mag`` is that sum over absolute values, ``rows`` its length.  Such sums can cancel: a convolution bias or weight in
    front of a BatchNorm (the norm removes a column's shift and scale, so the cotangent columns sum to zero), ``att_dst``
    (it shifts all logits of a target alike, which the softmax removes except across the leaky-ReLU's kink), the MinCUT
    losses (ratios, invariant to the scale of the assignment; softmax cotangent rows sum to zero).  Their float32 values
    are rounding residue of size ~ rows * 2^-24 * mag in ANY evaluation order, while max|grad| (the referee's scale) is
    arbitrarily smaller.  The bound for such a tensor is f64_close's

        |got - f64| <= 3 * n * 2^-24 * mag,     n = rows + chain,

    ``chain`` = the lengths of the sums on the paths through this parameter between the model's input and the loss:
    only modules whose output RECEIVED a cotangent count (a branch the loss does not see -- HSCN's virtual branch -- is
    on no such path; in the sequential models every layer is on the path of every parameter: its input passed through the
    layers before it, its cotangent through those after it).  Per module: fan-in + fan-out of a Linear, largest
    in-degree + 4 of a convolution call, H + 4 of a LayerNorm, rows + 4 of a BatchNorm; plus ``chain_extra``, what the
    caller adds for functions behind the last module (the pooled segment, the MinCUT contractions).  Nothing in it is
    measured from the code under test.

    Limits of the form, and why it is applied to named tensors only: ``mag`` takes the cotangent rows as carrying
    relative error, which understates the residue where a cotangent row is itself a cancelling sum; so a test may use
    it only for tensors it lists with their reason (``referee_all(cancelling=...)``) and must show its teeth there
    (``bound_teeth``): a reference with one edge removed is rejected by referee and bound together."""

    def __init__(self, model, chain_extra=0):
        from oracle import pyg_ops as P
        self.mag, self.rows, self.chain = {}, {}, float(chain_extra)
        self._handles, self._gats = [], []
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.Linear):
                self._handles.append(mod.register_forward_hook(self._linear(name)))
            elif isinstance(mod, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)):
                self._handles.append(mod.register_forward_hook(self._norm(name)))
            elif isinstance(mod, (P.GCNConv, P.GATConv, P.GraphConv)):
                self._handles.append(mod.register_forward_hook(self._conv(name)))
                if isinstance(mod, P.GATConv):
                    mod.term_hook = self._att(name)
                    self._gats.append(mod)

    def _add(self, key, mag, rows):
        self.mag[key] = self.mag.get(key, 0) + mag.detach()
        self.rows[key] = self.rows.get(key, 0) + int(rows)

    def _on_cotangent(self, out, length, record=None):
        """When ``out`` receives its cotangent: the module is on a path to the loss (its sums join ``chain``)."""
        def back(g):
            self.chain += length
            if record is not None:
                record(g.detach().abs())
        if out.requires_grad:
            out.register_hook(back)

    def _linear(self, name):
        def hook(mod, inp, out):
            x = inp[0].detach().abs().reshape(-1, inp[0].shape[-1])

            def record(g):
                g = g.reshape(-1, g.shape[-1])
                self._add(f"p.{name}.weight", g.t() @ x, g.shape[0])
                if mod.bias is not None:
                    self._add(f"p.{name}.bias", g.sum(0), g.shape[0])
            self._on_cotangent(out, mod.in_features + mod.out_features, record)
        return hook

    def _norm(self, name):
        def hook(mod, inp, out):
            xhat = ((out - mod.bias) / mod.weight).detach().abs()

            def record(g):
                self._add(f"p.{name}.weight", (g * xhat).sum(0), g.shape[0])
                self._add(f"p.{name}.bias", g.sum(0), g.shape[0])
            self._on_cotangent(out, (out.shape[0] if isinstance(mod, torch.nn.BatchNorm1d) else out.shape[1]) + 4, record)
        return hook

    def _conv(self, name):
        def hook(mod, inp, out):
            ei = inp[1]
            length = (int(torch.bincount(ei[1]).max()) if ei.numel() else 0) + 4
            has_bias = isinstance(getattr(mod, "bias", None), torch.Tensor)
            self._on_cotangent(out, length, (lambda g: self._add(f"p.{name}.bias", g.sum(0), g.shape[0])) if has_bias else None)
        return hook

    def _att(self, name):
        def term(a_src, a_dst, h_src, h_dst):
            for a, h, key in ((a_src, h_src, "att_src"), (a_dst, h_dst, "att_dst")):
                if a.requires_grad:
                    hh = h.detach().abs()
                    a.register_hook(lambda g, hh=hh, key=key: self._add(
                        f"p.{name}.{key}", (g.detach().abs().unsqueeze(-1) * hh).sum(0, keepdim=True), g.shape[0]))
        return term

    def close(self):
        for h in self._handles:
            h.remove()
        for m in self._gats:
            m.term_hook = None
        self._handles, self._gats = [], []

    def rename(self, f):
        self.mag = {f(k): v for k, v in self.mag.items()}
        self.rows = {f(k): v for k, v in self.rows.items()}

    def bound_holds(self, key, got, ref64, what=""):
        """f64_close(got, ref64, mag, rows + chain) for the parameter gradient ``key``; False where no terms were recorded."""
        if key not in self.mag:
            return False
        n = self.rows[key] + self.chain
        mag = self.mag[key].reshape(ref64.shape)
        lim = F64_C * n * U32 * float(mag.max())
        print(f"   a-priori {what} {key}: n = {self.rows[key]} rows + {self.chain:.0f} chain, max mag = {float(mag.max()):.3e}, "
              f"largest limit = {lim:.3e}")
        return f64_close(got, ref64, mag, n, what=f"{what} {key}")

    def bound_teeth(self, got, o32, o64, dropped64_list, keys, what=""):
        """Teeth of the combined criterion for the tensors ``keys`` that may take the bound: against the float64
        reference with one edge removed that changes the tensor most, the HIP result must be rejected by the referee
        AND by the bound (``mag`` and ``n`` as recorded for the true reference: the same bar)."""
        reached = most_changed(o64, dropped64_list)
        for k in keys:
            assert k in reached, f"{what} {k}: no removed edge reaches this tensor"
            d, full = reached[k].detach().cpu().double(), o64[k].detach().cpu().double()
            r = referee(got[k], _shifted(o32, k, full, d), d, f"{what} {k} [one edge dropped]")
            assert r > 1.0, f"{what} {k}: the referee cannot see a dropped edge (ratio {r:.3f})"
            assert not self.bound_holds(k, got[k], d, what + " [one edge dropped]"), \
                f"{what} {k}: the a-priori bound cannot see a dropped edge"


def grads_of(model, **inputs):
    """{"p.<name>": parameter gradient or None, "x.<name>": input gradient}: the dict ``referee_all`` compares."""
    res = {"x." + k: v.grad for k, v in inputs.items()}
    if model is not None:
        res.update({"p." + n: p.grad for n, p in model.named_parameters()})
    return {k: (None if v is None else v.detach().clone()) for k, v in res.items()}


def oracle_twin(om, step, dtype=torch.float64, gates=None, chain_extra=None, steps=1, guard=True):
    """One evaluation of the oracle ``om`` in ``dtype`` from a copy (``copy.deepcopy(om).to(dtype)``: identical weights):
    ``step(model, dtype)`` does one forward + backward and returns the dict of its input gradients ({} if none);
    ``steps`` passes from the initial state (running statistics), the last one's results.  On the last pass the kink
    guard is hooked (``gates(model)``: modules whose output feeds a ReLU; the oracle's GATConv logits are found by
    themselves) and, when ``chain_extra`` is given, ``TermMagnitudes`` records.
    Returns (gradients {"x.<name>" / "p.<name>"}, guard or None, terms or None)."""
    import copy
    m = copy.deepcopy(om).to(dtype)
    m.train(om.training)
    kg, terms, xg = (KinkGuard() if guard else None), None, {}
    for s in range(steps):
        m.zero_grad(set_to_none=True)
        if s == steps - 1:
            if kg is not None:
                kg.attach(m)
                for g in (gates(m) if gates is not None else []):
                    kg.relu_after(g)
            if chain_extra is not None:
                terms = TermMagnitudes(m, chain_extra)
        xg = step(m, dtype) or {}
    if kg is not None:
        kg.close()
    if terms is not None:
        terms.close()
    res = {"x." + k: (None if v is None else v.detach().clone()) for k, v in xg.items()}
    res.update({"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()})
    return res, kg, terms


def scn_step_in_dtype(m, x, edge_index):
    """``oracle.models.scn_step_single_graph`` in the dtype of ``m``'s parameters (for the float64 twin): the stage-A
    body gcn_norm(add_self_loops=True) -> message passing -> MLP -> dense_mincut_pool, with the dense adjacency --
    integer counts, exact in any float type -- cast to that dtype (``to_dense_adj`` itself returns float32).
    Returns (softmax assignment, mincut loss, orthogonality loss)."""
    from oracle import pyg_ops as P
    dt = m.mp.module_0.lin_rel.weight.dtype
    ei2, ew = P.gcn_norm(edge_index, None, x.size(0), add_self_loops=True, dtype=dt)
    h = m.mp(x.to(dt), ei2, ew)
    s = m._run_mlp(h)
    _, _, mc, o = P.dense_mincut_pool(h, P.to_dense_adj(ei2).to(dt), s)
    return torch.softmax(s, dim=-1), mc, o


# --------------------------------------------------------------------------- #
# half-precision STORAGE against float64 (tests/test_gpu_f16_edges.py): the window a correctly rounded store must fall
# into, and an oracle forced onto the stored values so that a rounding flip cannot propagate
# --------------------------------------------------------------------------- #
def to_half(t):
    """float64 (or float32) -> IEEE half in ONE round-to-nearest-even step (numpy converts the double's bits directly;
    double -> float -> half would round twice and can cross a tie).  Overflow gives inf, NaN stays NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(t.detach().cpu().numpy().astype(np.float16))


def half_window(r64, o32):
    """The halves a correct store of the tensor may hold.  ``r64``: the float64 oracle's value BEFORE storage, ``o32``
    the float32 oracle's from the same inputs.  With ``referee``'s bar unchanged, b = 2 max|o32 - r64| + 8 * 2^-23 *
    max|r64|, a float32 evaluation d32 with |d32 - r64| <= b stores half(d32), and rounding is monotone:

        half(r64 - b)  <=  stored  <=  half(r64 + b)          element by element,

    both ends rounded once (``to_half``).  Returns (lo, hi, b): half tensors and the bar."""
    r = r64.detach().cpu().double()
    b = 2.0 * float((o32.detach().cpu().double() - r).abs().max()) + 8.0 * 2.0 ** -23 * float(r.abs().max()) \
        if r.numel() else 0.0
    return to_half(r - b), to_half(r + b), b


def in_half_window(d, lo, hi):
    """Element-wise verdict for stored halves ``d``: lo <= d <= hi, an infinite end admits (lo = +inf: demands) an
    infinity of its sign, and where the window is NaN the stored value must be NaN."""
    d, lo, hi = d.detach().cpu().double(), lo.double(), hi.double()
    nan = torch.isnan(lo) | torch.isnan(hi)
    return torch.where(nan, torch.isnan(d), (lo <= d) & (d <= hi))


def window_shares(r64, lo, hi, b):
    """How sharp the window is, over the positive elements of ``r64``: the share determined to the bit (lo == hi), the
    share whose window spans more than two adjacent halves (among those with r64 - b > 0, where the bit patterns of
    both ends are ordered like their values), the share that are half subnormals (0 < r64 < 2^-14)."""
    r = r64.detach().cpu().double()
    pos = r > 0
    if not bool(pos.any()):
        return dict(determined=1.0, wide=0.0, subnormal=0.0, positive=0)
    span = (hi.view(torch.int16).int() - lo.view(torch.int16).int())[pos & (r - b > 0) & torch.isfinite(hi.double())]
    return dict(determined=float((lo == hi)[pos].double().mean()),
                wide=float((span > 1).double().mean()) if span.numel() else 0.0,
                subnormal=float((r[pos] < 2.0 ** -14).double().mean()), positive=int(pos.sum()))


class ForcedStore:
    """A ``store`` callable for ``oracle.models.HSCN.forward`` / ``SCN.forward`` (tagged: it is told which tensor it is
    handed) that FORCES the oracle onto the values the device stored: ``forced[(name, layer)]`` replaces the tensor's
    value, t + (forced - t).detach(), and the gradient passes straight through -- the HIP backward treats the stored
    value as the activation.  The float32 and the float64 oracle then see the very activations the kernel's backward
    read, so a rounding flip of one evaluation cannot reach the next layer.  Tensors without a forced value (input
    features, which are halves already, and the virtual rows, which never reach the prediction) round as
    ``oracle.models.half_storage`` does."""
    tagged = True

    def __init__(self, forced):
        self.forced = {k: v.detach().cpu() for k, v in forced.items()}

    def __call__(self, t, name, layer):
        f = self.forced.get((name, layer))
        if f is None:
            return t + (to_half(t).to(t.dtype) - t).detach()
        assert f.shape == t.shape, (name, layer, tuple(f.shape), tuple(t.shape))
        return t + (f.to(t.dtype) - t).detach()
