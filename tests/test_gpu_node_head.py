"""hscn_node_head_fwd / hscn_node_head_bwd (csrc/node_head.hip; graph_hscn.nn.head) against float64 torch on the CPU,
and the layered ``Linear`` pair under the same bounds on the same inputs.

Bounds: ``tests/helpers.check_f64`` with ``F64_C`` as it is; n and mag as its docstring prescribes (a linear op: the
length of the sum and the same op on absolute values; an activation: n gains 4, mag gains |y|), chained:
  hidden  h = act(b1 + x W1^T):            n_h = H + 5,              hm = |x| |W1|^T + |b1| + |h|
  pred    = b2 + h W2^T:                   n = (H + 1) + n_h,        mag = hm |W2|^T + |b2|        (hm >= |h|)
  g       = scale * g_pred (one rounding, counted in every n below)
  g_pre   = (g W2) act'(h), |act'| <= 1 and act' 1-Lipschitz in h for the four activations:
                                           n_p = C + 2 + n_h,        pm = (|g| |W2|) (1 + hm)
  g_x     = g_pre W1:                      n = H + n_p,              mag = pm |W1|
  gW1     = g_pre^T x, gb1 = sum g_pre:    n = N + n_p (+1 accumulate), mag = pm^T |x|, sum pm      (+ |existing|)
  gW2     = g^T h, gb2 = sum g:            n = N + 1 + n_h (+1),     mag = |g|^T hm, sum |g|       (+ |existing|)
Dropped terms: pred and g_x without their largest product (``drop_largest_product``), the weight gradients without
the row of the largest contribution.  A bias gradient is a plain sum over N rows whose mag adds absolute values over
the C (and H) terms behind every row: one row out of several hundred is below what any a-priori bound of a sum that
long resolves, so beyond one wave of rows the term dropped is the chunk the kernel's row walk handles at a time --
the 64 rows of the sub-tile that holds the largest row.  That a SINGLE row cannot go missing from a bias sum is shown
where the bound can resolve it: ``test_a_single_row_cannot_go_missing_from_the_bias_sums`` gives one row an upstream
gradient as large as all the others' together and drops exactly that row.

A ReLU whose pre-activation is within rounding of zero has no float64 derivative to compare with: the inputs are
redrawn (next seed) until every |pre-activation| > 1e-5, far above the ~1e-6 the float32 chain can be off by at
these magnitudes.

Shapes: a lane owns a row and a workgroup 256 of them (hscn_node_head_rows_per_workgroup): N = 1, around a wave,
around a workgroup, three workgroups and a partial one (the fold adds four rows of partials)."""
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import check_f64, drop_largest_product

pytestmark = pytest.mark.gpu

DEV = "cuda"
RPW = 256
N_EDGES = [1, 63, 64, 65, RPW - 1, RPW + 1, 3 * RPW + 5]
H_EDGES = [16, 32, 64]
C_EDGES = [1, 2, 21, 64]
ACTS = ["relu", "elu", "tanh", "identity"]
ACT64 = {"relu": torch.relu, "elu": F.elu, "tanh": torch.tanh, "identity": lambda t: t}


class _Case:
    """Seeded inputs and every float64 reference, computed once on the CPU."""

    def __init__(self, N, H, C, act, seed, scale=1.0, existing=False, dominant_row=None):
        for attempt in range(50):
            g = torch.Generator().manual_seed(seed + 1000 * attempt)
            self.x = torch.randn(N, H, generator=g)
            self.W1 = torch.randn(H, H, generator=g) / H ** 0.5
            self.b1 = 0.5 * torch.randn(H, generator=g)
            self.W2 = torch.randn(C, H, generator=g) / H ** 0.5
            self.b2 = 0.5 * torch.randn(C, generator=g)
            self.g_pred = torch.randn(N, C, generator=g) / N
            if dominant_row is not None:
                self.g_pred[dominant_row] *= N
            self.old = [torch.randn(s, generator=g) for s in ((H, H), (H,), (C, H), (C,))] if existing else None
            pre = self.x.double() @ self.W1.double().T + self.b1.double()
            if act != "relu" or float(pre.abs().min()) > 1e-5:
                break
        else:
            raise AssertionError("no draw keeps the ReLU away from zero")
        self.N, self.H, self.C, self.act, self.scale = N, H, C, act, scale
        p = [t.double().requires_grad_(True) for t in (self.x, self.W1, self.b1, self.W2, self.b2)]
        x, W1, b1, W2, b2 = p
        h = ACT64[act](x @ W1.T + b1)
        pred = h @ W2.T + b2
        g32 = (torch.tensor(scale) * self.g_pred) if scale != 1.0 else self.g_pred      # the kernel's one rounding
        g = g32.double()
        self.grads = list(torch.autograd.grad(pred, p, g))
        self.pred, self.h, self.g = pred.detach(), h.detach(), g
        ax, aW1, aW2 = x.detach().abs(), W1.detach().abs(), W2.detach().abs()
        self.hm = ax @ aW1.T + b1.detach().abs() + self.h.abs()
        self.pm = (g.abs() @ aW2) * (1.0 + self.hm)
        # g_pre in float64, for the dropped terms: d pred / d (pre-activation)
        z = (x.detach() @ W1.detach().T + b1.detach()).requires_grad_(True)
        (self.gpre,) = torch.autograd.grad(ACT64[act](z) @ W2.detach().T, z, g)
        if existing:
            for i in range(4):
                self.grads[1 + i] = self.grads[1 + i] + self.old[i].double()

    def dev(self):
        return [t.to(DEV) for t in (self.x, self.W1, self.b1, self.W2, self.b2)]

    def check_pred(self, got, what):
        H = self.H
        W2t = self.W2.double().T
        dropped = drop_largest_product(self.pred, self.h, W2t, post=lambda r, o, t: float(self.pred[r, o]) - t)
        check_f64(got, self.pred, self.hm @ W2t.abs() + self.b2.double().abs(), 2 * H + 6, dropped, what=f"{what} pred")

    def check_grads(self, got, what, gx=True, bias_row=False):
        """``bias_row``: the bias gradients' dropped term is the single largest row, not its sub-tile."""
        chunk = (lambda t, r: t[r]) if bias_row else _chunk
        N, H, C = self.N, self.H, self.C
        n_h, acc = H + 5, 1 if self.old is not None else 0
        n_p = C + 2 + n_h
        old = [o.double().abs() for o in self.old] if self.old is not None else [0.0] * 4
        g_x, gW1, gb1, gW2, gb2 = got
        rx, rW1, rb1, rW2, rb2 = self.grads
        W1 = self.W1.double()
        if gx:
            check_f64(g_x, rx, self.pm @ W1.abs(), H + n_p, drop_largest_product(rx, self.gpre, W1), what=f"{what} g_x")
        x, h, g, gpre = self.x.double(), self.h, self.g, self.gpre
        r1 = int((gpre.abs().max(1).values * x.abs().max(1).values).argmax())         # the row of the largest term
        check_f64(gW1, rW1, self.pm.T @ x.abs() + old[0], N + n_p + acc, rW1 - torch.outer(gpre[r1], x[r1]),
                  what=f"{what} gW1")
        rb = int(gpre.abs().max(1).values.argmax())
        check_f64(gb1, rb1, self.pm.sum(0) + old[1], N + n_p + acc, rb1 - chunk(gpre, rb), what=f"{what} gb1")
        r2 = int((g.abs().max(1).values * h.abs().max(1).values).argmax())
        if float(h.abs().max()) > 0.0:
            check_f64(gW2, rW2, g.abs().T @ self.hm + old[2], N + 1 + n_h + acc, rW2 - torch.outer(g[r2], h[r2]),
                      what=f"{what} gW2")
        rg = int(g.abs().max(1).values.argmax())
        check_f64(gb2, rb2, g.abs().sum(0) + old[3], N + 1 + acc, rb2 - chunk(g, rg), what=f"{what} gb2")


def _chunk(t, r):
    """The column sums of the 64-row sub-tile that holds row ``r`` (the row itself up to one wave of rows)."""
    if t.size(0) <= 64:
        return t[r]
    return t[r - r % 64:r - r % 64 + 64].sum(0)


def _combos(H):
    """Every C and every activation once per (N, H), paired differently for each H."""
    k = H_EDGES.index(H)
    return [(C_EDGES[i], ACTS[(i + k) % 4]) for i in range(4)]


def test_the_row_tile_is_what_the_shapes_assume():
    from graph_hscn.nn import head
    assert head.rows_per_workgroup() == RPW
    from graph_hscn._hip import lib
    for N, wgs in ((1, 1), (RPW, 1), (RPW + 1, 2), (3 * RPW + 5, 4), (256 * RPW + 1, 256)):
        assert lib().hscn_node_head_workspace_bytes(N, 16, 10) == wgs * (16 + 10) * 17 * 4


@pytest.mark.parametrize("H", H_EDGES)
@pytest.mark.parametrize("N", N_EDGES)
def test_forward_and_backward_against_float64(N, H):
    from graph_hscn._hip import ACT
    from graph_hscn.nn import head
    for C, act in _combos(H):
        case = _Case(N, H, C, act, seed=17 * N + H + C)
        what = f"N={N} H={H} C={C} {act}"
        x, W1, b1, W2, b2 = case.dev()
        assert head.node_head_supported(H, C)
        pred = head.node_head_fwd_raw(x, W1, b1, W2, b2, ACT[act])
        case.check_pred(pred, what)
        got = head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), None, ACT[act])
        case.check_grads(got, what)
        again = head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), None, ACT[act])
        assert torch.equal(pred, head.node_head_fwd_raw(x, W1, b1, W2, b2, ACT[act]))
        for a, b in zip(got, again):
            assert torch.equal(a, b), what                                             # the same bits


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C", C_EDGES)
def test_every_class_width_with_every_activation(C, act):
    from graph_hscn._hip import ACT
    from graph_hscn.nn import head
    N, H = RPW + 1, 32
    case = _Case(N, H, C, act, seed=5 * C + len(act))
    what = f"product N={N} H={H} C={C} {act}"
    x, W1, b1, W2, b2 = case.dev()
    case.check_pred(head.node_head_fwd_raw(x, W1, b1, W2, b2, ACT[act]), what)
    case.check_grads(head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), None, ACT[act]), what)


@pytest.mark.parametrize("N,H,C,act,row", [(3 * RPW + 5, 64, 64, "elu", 700), (3 * RPW + 5, 16, 10, "relu", 300),
                                           (RPW + 1, 32, 21, "tanh", RPW), (RPW - 1, 16, 2, "identity", 130)])
def test_a_single_row_cannot_go_missing_from_the_bias_sums(N, H, C, act, row):
    """Row ``row`` (in the last partial workgroup, in a middle sub-tile, the one row of the second workgroup, ...)
    carries an upstream gradient N times the others': the bias bounds resolve it, and it is the row dropped."""
    from graph_hscn._hip import ACT
    from graph_hscn.nn import head
    case = _Case(N, H, C, act, seed=N + row, dominant_row=row)
    assert int(case.g.abs().max(1).values.argmax()) == row
    x, W1, b1, W2, b2 = case.dev()
    got = head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), None, ACT[act])
    case.check_grads(got, f"dominant row N={N} H={H} C={C} {act}", bias_row=True)


@pytest.mark.parametrize("N,H,C,act", [(65, 16, 21, "relu"), (RPW + 1, 32, 2, "tanh"), (3 * RPW + 5, 64, 64, "elu"),
                                       (3 * RPW + 5, 16, 10, "identity")])
def test_scale_and_accumulate(N, H, C, act):
    from graph_hscn._hip import ACT
    from graph_hscn.nn import head
    case = _Case(N, H, C, act, seed=N + C, scale=-2.5, existing=True)
    x, W1, b1, W2, b2 = case.dev()
    grads = tuple(o.to(DEV) for o in case.old)
    scale = torch.tensor([-2.5], device=DEV)
    got = head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), scale, ACT[act], grads=grads, accumulate=True)
    case.check_grads(got, f"scale+accumulate N={N} H={H} C={C} {act}")
    # without g_x, into given buffers, not accumulating: the buffers' old contents do not matter
    plain = _Case(N, H, C, act, seed=N + C, scale=-2.5)
    got = head.node_head_bwd_raw(x, W1, b1, W2, b2, case.g_pred.to(DEV), scale, ACT[act], want_gx=False, grads=grads)
    assert got[0] is None
    plain.check_grads(got, f"scale N={N} H={H} C={C} {act}", gx=False)


@pytest.mark.parametrize("route", ["fused", "layered"])
@pytest.mark.parametrize("N,H,C,act", [(RPW - 1, 16, 10, "relu"), (3 * RPW + 5, 32, 21, "elu"), (65, 64, 64, "tanh")])
def test_the_module_routes_pass_the_same_bound_with_dense_and_lazy_gradients(N, H, C, act, route, monkeypatch):
    from graph_hscn.loss import LazyScaled, criterion
    from graph_hscn.nn import Linear
    from graph_hscn.nn.head import NodeHead
    case = _Case(N, H, C, act, seed=3 * N + H)
    lin_1, lin_2 = Linear(H, H).to(DEV), Linear(H, C).to(DEV)
    with torch.no_grad():
        for p, v in zip((lin_1.weight, lin_1.bias, lin_2.weight, lin_2.bias), (case.W1, case.b1, case.W2, case.b2)):
            p.copy_(v)
    head = NodeHead(lin_1, lin_2, act, route=route)
    params = [lin_1.weight, lin_1.bias, lin_2.weight, lin_2.bias]
    what = f"{route} N={N} H={H} C={C} {act}"
    # a dense upstream gradient
    x = case.x.to(DEV).requires_grad_(True)
    pred = head(x)
    assert head.last_route == route
    case.check_pred(pred, what)
    got = torch.autograd.grad(pred, [x] + params, case.g_pred.to(DEV))
    case.check_grads(got, f"{what} dense")
    # the criterion's LazyScaled gradient, root 2.5: the reference takes the criterion's own float32 gradient
    target = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(N))
    probe = pred.detach().requires_grad_(True)
    (2.5 * criterion("weighted_cross_entropy", probe, target.to(DEV))[0]).backward()
    lazy = _Case(N, H, C, act, seed=3 * N + H)
    lazy.g_pred = probe.grad.cpu()                    # = 2.5 * grad, rounded once, as the launch forms it
    lazy.__dict__.update(_with_gradient(lazy, lazy.g_pred))
    calls = []
    real = LazyScaled.materialize
    monkeypatch.setattr(LazyScaled, "materialize", lambda self: calls.append(1) or real(self))
    x = case.x.to(DEV).requires_grad_(True)
    loss, _ = criterion("weighted_cross_entropy", head(x), target.to(DEV))
    got = torch.autograd.grad(2.5 * loss, [x] + params)
    assert bool(calls) == (route == "layered")        # the fused backward consumes it unmultiplied
    if float(lazy.g.abs().max()) > 0.0:               # (C = 1 has a zero gradient: nothing to bound)
        lazy.check_grads(got, f"{what} lazy")


def _with_gradient(case, g_pred):
    """The references of ``case`` for another upstream gradient."""
    fresh = _Case.__new__(_Case)
    fresh.__dict__.update(case.__dict__)
    p = [t.double().requires_grad_(True) for t in (case.x, case.W1, case.b1, case.W2, case.b2)]
    x, W1, b1, W2, b2 = p
    h = ACT64[case.act](x @ W1.T + b1)
    pred = h @ W2.T + b2
    g = g_pred.double()
    grads = list(torch.autograd.grad(pred, p, g))
    z = (x.detach() @ W1.detach().T + b1.detach()).requires_grad_(True)
    (gpre,) = torch.autograd.grad(ACT64[case.act](z) @ W2.detach().T, z, g)
    pm = (g.abs() @ W2.detach().abs()) * (1.0 + case.hm)
    return dict(g=g, grads=grads, gpre=gpre, pm=pm)


def test_a_misaligned_view_is_refused_by_the_launch_and_copied_by_the_wrapper():
    from graph_hscn import _hip
    from graph_hscn.nn.head import NodeHeadFn, node_head_fwd_raw
    g = torch.Generator().manual_seed(0)
    N, H, C = 70, 16, 5
    flat = torch.randn(1 + N * H, generator=g).to(DEV)
    x = flat[1:].view(N, H)                              # contiguous, 4 bytes past a 16-byte boundary
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    W1, b1 = torch.randn(H, H, generator=g).to(DEV), torch.randn(H, generator=g).to(DEV)
    W2, b2 = torch.randn(C, H, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    p = _hip.ptr
    pred = torch.empty(N, C, device=DEV)
    assert _hip.lib().hscn_node_head_fwd(p(x), p(W1), p(b1), p(W2), p(b2), N, H, C, 1, p(pred), None) == -1
    assert _hip.lib().hscn_node_head_bwd(p(x), p(W1), p(b1), p(W2), p(b2), p(pred), None, N, H, C, 1, None, p(W1), p(b1),
                                         p(W2), p(b2), 0, p(flat), flat.numel() * 4, None) == -1
    want = node_head_fwd_raw(x.clone(), W1, b1, W2, b2, 1)
    xr = x.detach().requires_grad_(True)
    got = NodeHeadFn.apply(xr, W1, b1, W2, b2, 1)
    assert torch.equal(got, want)
    got.sum().backward()
    assert xr.grad.shape == x.shape
    torch.cuda.synchronize()


def test_outside_the_envelope_the_launches_refuse_and_the_wrapper_goes_layered():
    from graph_hscn import _hip
    from graph_hscn.nn import Linear
    from graph_hscn.nn.head import NodeHead
    L = _hip.lib()
    p = _hip.ptr(torch.zeros(4096, device=DEV))
    assert L.hscn_node_head_fwd(p, p, p, p, p, 4, 24, 4, 0, p, None) == -3
    assert L.hscn_node_head_fwd(p, p, p, p, p, 4, 16, 65, 0, p, None) == -3
    assert L.hscn_node_head_bwd(p, p, p, p, p, p, None, 4, 16, 4, 0, p, p, p, p, p, 0, p, 4, None) == -2
    lin_1, lin_2 = Linear(24, 24).to(DEV), Linear(24, 5).to(DEV)
    head = NodeHead(lin_1, lin_2, "relu")
    x = torch.randn(10, 24, device=DEV)
    want = lin_2(lin_1(x, act="relu"))
    assert torch.equal(head(x), want) and head.last_route == "layered"
    with pytest.raises(RuntimeError, match="hscn_node_head_supported"):
        NodeHead(lin_1, lin_2, "relu", route="fused")(x)
    torch.cuda.synchronize()
