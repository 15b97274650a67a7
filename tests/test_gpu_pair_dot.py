"""hscn_pair_dot_fwd / hscn_pair_dot_bwd (csrc/edge_head.hip; graph_hscn.nn.head.pair_dot) against float64 torch on the
CPU.

Bounds: ``tests/helpers.check_f64`` with ``F64_C`` as it is.
  score[p] = sum_k z[u, k] z[v, k]:  n = D, mag = sum_k |z[u, k]| |z[v, k]|; dropped term: the largest product.
  g_z[i]   = sum over the incidences of i of g_p z[other]:  n = deg_i + 1, mag = sum |g_p| |z[other]|; dropped term:
             the largest incidence.  With ``scale`` the reference multiplies in float32 first, which is the kernel's own
             one rounding of g_p.  A node of degree 0 must be exactly zero.

Shapes: a lane group of D / 4 lanes (rounded up to a power of two) owns a pair, so a workgroup holds
hscn_pair_dot_pairs_per_workgroup(D) pairs: P = 1, around a wave's worth of lanes, around a workgroup, three workgroups
and a partial one; N = 70 (two workgroups of nodes in the backward at D = 64, where a workgroup holds 16)."""
import pytest
import torch

from tests.helpers import check_f64

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 70
D_EDGES = [4, 12, 16, 32, 64]


def _p_edges(D):
    from graph_hscn.nn.head import pairs_per_workgroup
    per = pairs_per_workgroup(D)
    assert per == 256 // max(1, 1 << (D // 4 - 1).bit_length())
    return [1, 63, 64, 65, per - 1, per + 1, 3 * per + 5]


class _Case:
    """Seeded inputs and the float64 references, computed once on the CPU."""

    def __init__(self, D, pairs, seed, scale=None, n=N):
        g = torch.Generator().manual_seed(seed)
        self.z = torch.randn(n, D, generator=g)
        self.pairs = pairs                                             # int64 [2, P]
        P = pairs.size(1)
        self.g = torch.randn(P, generator=g) / max(P, 1)
        self.scale = scale
        z64, (u, v) = self.z.double(), pairs
        self.score = (z64[u] * z64[v]).sum(1)
        self.score_mag = (z64[u].abs() * z64[v].abs()).sum(1)
        prod = (z64[u] * z64[v])
        self.score_dropped = self.score.clone()
        if P:
            p = int(prod.abs().max(1).values.argmax())
            self.score_dropped[p] -= prod[p][prod[p].abs().argmax()]
        g32 = self.g * torch.tensor(scale) if scale is not None else self.g      # the kernel's one rounding of g_p
        g64 = g32.double()
        self.gz = torch.zeros(n, D, dtype=torch.float64)
        self.gz.index_add_(0, u, g64[:, None] * z64[v])
        self.gz.index_add_(0, v, g64[:, None] * z64[u])
        self.gz_mag = torch.zeros(n, D, dtype=torch.float64)
        self.gz_mag.index_add_(0, u, g64.abs()[:, None] * z64[v].abs())
        self.gz_mag.index_add_(0, v, g64.abs()[:, None] * z64[u].abs())
        self.deg = torch.bincount(u, minlength=n) + torch.bincount(v, minlength=n)
        self.gz_dropped = self.gz.clone()
        if P:
            size = g64.abs() * torch.maximum(z64[u].abs().max(1).values, z64[v].abs().max(1).values)
            p = int(size.argmax())
            if float(z64[u[p]].abs().max()) >= float(z64[v[p]].abs().max()):
                self.gz_dropped[v[p]] -= g64[p] * z64[u[p]]            # the incidence of v_p: its other end is u_p
            else:
                self.gz_dropped[u[p]] -= g64[p] * z64[v[p]]

    def run(self):
        from graph_hscn.nn.head import PairStructure, pair_dot_bwd_raw, pair_dot_fwd_raw
        z, pairs, g = self.z.to(DEV), self.pairs.to(DEV), self.g.to(DEV)
        st = PairStructure(pairs, z.size(0))
        flags = torch.zeros(1, dtype=torch.int32, device=DEV)
        score = pair_dot_fwd_raw(z, st.index32, flags)
        scale = torch.tensor([self.scale], device=DEV) if self.scale is not None else None
        gz = pair_dot_bwd_raw(z, st, g, scale)
        return score, gz, flags

    def check(self, score, gz, what):
        D = self.z.size(1)
        check_f64(score, self.score, self.score_mag, D, self.score_dropped, what=f"{what} score")
        check_f64(gz, self.gz, self.gz_mag, (self.deg + 1)[:, None], self.gz_dropped, what=f"{what} g_z")
        none = self.deg == 0
        assert bool((gz.cpu()[none] == 0).all()), f"{what}: a node without incidences must get an exact zero row"


def _random_pairs(P, seed, n=N):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n, (2, P), generator=g)


@pytest.mark.parametrize("D", D_EDGES)
def test_forward_and_backward_against_float64_at_the_pair_count_edges(D):
    for k, P in enumerate(_p_edges(D)):
        case = _Case(D, _random_pairs(P, 100 + k), seed=D * 100 + k, scale=None if k % 2 else 0.37)
        score, gz, flags = case.run()
        assert int(flags.item()) == 0
        case.check(score, gz, f"D={D} P={P}")


def _structured_pairs():
    """A hub (node 0) with 130 incidences -- more than two waves' worth of entries for the widest lane group -- 65 as
    source and 65 as target; nodes 62..69 with none; a pair (i, i); node 61 source in one pair and target in another."""
    hub_out = torch.stack([torch.zeros(65, dtype=torch.int64), 1 + torch.arange(65) % 59])
    hub_in = torch.stack([1 + (torch.arange(65) * 7) % 59, torch.zeros(65, dtype=torch.int64)])
    rest = torch.tensor([[60, 61, 11, 13, 13], [60, 11, 61, 2, 2]])    # (60, 60); 61 -> 11 and 11 -> 61; a repeated pair
    pairs = torch.cat([hub_out, rest, hub_in], 1)
    return pairs[:, torch.randperm(pairs.size(1), generator=torch.Generator().manual_seed(3))]


@pytest.mark.parametrize("D", D_EDGES)
@pytest.mark.parametrize("scale", [None, -2.5])
def test_structure_cases_hub_isolated_nodes_self_pair(D, scale):
    pairs = _structured_pairs()
    case = _Case(D, pairs, seed=7 + D, scale=scale)
    assert int(case.deg[0]) == 130 and int(case.deg[62:].sum()) == 0 and int(case.deg[60]) == 2
    score, gz, flags = case.run()
    assert int(flags.item()) == 0
    case.check(score, gz, f"structured D={D} scale={scale}")
    # the pair (60, 60) contributes 2 g z[60] through its two incidences
    p = int(((pairs[0] == 60) & (pairs[1] == 60)).nonzero()[0])
    g = case.g[p] * torch.tensor(scale) if scale is not None else case.g[p]
    want = 2.0 * g.double() * case.z[60].double()
    assert torch.allclose(gz[60].cpu().double(), want, rtol=1e-6, atol=0.0)


def test_two_calls_give_the_same_bits():
    case = _Case(64, _structured_pairs(), seed=11, scale=0.5)
    a, b = case.run(), case.run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_score_does_not_depend_on_where_the_pair_sits():
    """The same pair anywhere in the list, in any lane group of any wave, gives the same bits: the metric kernel's ties
    rely on it."""
    from graph_hscn.nn.head import pair_dot
    for D in D_EDGES:
        g = torch.Generator().manual_seed(D)
        z = torch.randn(N, D, generator=g).to(DEV)
        one = torch.tensor([[3], [17]], device=DEV)
        many = one.repeat(1, 700)
        s1, sm = pair_dot(z, one), pair_dot(z, many)
        assert bool((sm == s1[0]).all())
        assert torch.equal(pair_dot(z, one.flip(0)), s1)               # <z_u, z_v> = <z_v, z_u>, bit for bit


def test_autograd_route_no_pairs_and_the_lazy_scale(monkeypatch):
    from graph_hscn.loss import criterion
    from graph_hscn.nn import head
    from graph_hscn.nn.head import PairStructure, pair_dot
    case = _Case(16, _random_pairs(200, 5), seed=21)
    z = case.z.to(DEV).requires_grad_(True)
    score = pair_dot(z, case.pairs.to(DEV))
    score.backward(case.g.to(DEV))
    case.check(score.detach(), z.grad, "autograd")
    # P = 0: nothing is launched, the score is empty and the gradient zero
    z2 = case.z.to(DEV).requires_grad_(True)
    empty = pair_dot(z2, torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    assert empty.shape == (0,) and empty.dtype == torch.float32
    empty.sum().backward()
    assert z2.grad.shape == z2.shape and bool((z2.grad == 0).all())
    # the BCE criterion on a 1-D score: one device launch, and its LazyScaled gradient arrives unmultiplied
    label = (torch.rand(200, generator=torch.Generator().manual_seed(1)) < 0.3).float()
    z3 = case.z.to(DEV).requires_grad_(True)
    pairs3 = case.pairs.to(DEV)
    st = PairStructure(pairs3, N)
    s3 = pair_dot(z3, pairs3, st)
    loss, sig = criterion("cross_entropy", s3, label.to(DEV))
    seen = []
    raw = head.pair_dot_bwd_raw
    monkeypatch.setattr(head, "pair_dot_bwd_raw", lambda z, s, g, scale: seen.append(scale) or raw(z, s, g, scale))
    (3.0 * loss).backward()
    assert len(seen) == 1 and seen[0] is not None and float(seen[0]) == 3.0        # the scalar came in unmultiplied
    # a structure that belongs to other pairs or another node count is refused
    with pytest.raises(ValueError, match="another pair_index"):
        pair_dot(z3, pairs3.clone(), st)
    with pytest.raises(ValueError, match="nodes"):
        pair_dot(z3[:-1], pairs3, st)
    z64 = case.z.double().requires_grad_(True)
    u, v = case.pairs
    s64 = (z64[u] * z64[v]).sum(1)
    l64 = 3.0 * torch.nn.functional.binary_cross_entropy_with_logits(s64, label.double())
    l64.backward()
    assert abs(float(loss) * 3.0 - float(l64)) < 1e-5
    assert torch.allclose(sig.cpu().double(), torch.sigmoid(s64.detach()), atol=1e-6)
    assert torch.allclose(z3.grad.cpu().double(), z64.grad, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("D", [6, 68])
def test_widths_outside_the_envelope_are_refused(D):
    from graph_hscn.nn.head import pair_dot
    z = torch.zeros(N, D, device=DEV)
    with pytest.raises(RuntimeError, match="hscn_pair_dot_supported"):
        pair_dot(z, torch.zeros(2, 3, dtype=torch.int64, device=DEV))


def test_ids_out_of_range_score_zero_raise_the_flag_and_touch_nothing_else():
    """-1 and N, on a z that is a view into a buffer with one spare row on either side (filled with large values):
    even an unguarded read would stay inside the allocation -- and would show."""
    from graph_hscn.nn import head
    D = 16
    g = torch.Generator().manual_seed(5)
    buf = torch.full((N + 2, D), 1.0e3)
    buf[1:N + 1] = torch.randn(N, D, generator=g)
    buf = buf.to(DEV)
    z = buf[1:N + 1]
    assert z.is_contiguous() and z.data_ptr() % 16 == 0
    good = _random_pairs(300, 9)
    bad = good.clone()
    where = [0, 63, 64, 150, 299]
    bad[0, where[0]], bad[1, where[1]], bad[0, where[2]], bad[1, where[3]] = -1, N, N, -1
    bad[:, where[4]] = torch.tensor([N, -1])
    head.pair_flags(DEV).zero_()
    z_good = z.detach().clone().requires_grad_(True)
    s_good = head.pair_dot(z_good, good.to(DEV))
    assert int(head.pair_flags(DEV).item()) == 0
    z_bad = z.detach().requires_grad_(True)
    s_bad = head.pair_dot(z_bad, bad.to(DEV))
    assert int(head.pair_flags(DEV).item()) & head.PAIR_ID_OUT_OF_RANGE
    with pytest.raises(IndexError):
        head.check_pair_ids(DEV)
    head.check_pair_ids(DEV)                                           # read and cleared
    keep = torch.ones(300, dtype=torch.bool)
    keep[where] = False
    assert bool((s_bad.detach().cpu()[~keep] == 0).all())
    assert torch.equal(s_bad.detach().cpu()[keep], s_good.detach().cpu()[keep])
    # the backward leaves the offending pairs out: the gradient is that of the list without them
    gs = torch.randn(300, generator=g).to(DEV)
    s_bad.backward(gs)
    z_ref = z.detach().clone().requires_grad_(True)
    head.pair_dot(z_ref, good[:, keep].to(DEV)).backward(gs[keep.to(DEV)])
    assert torch.equal(z_bad.grad, z_ref.grad)
    assert bool(torch.isfinite(z_bad.grad).all()) and float(z_bad.grad.abs().max()) < 1.0e2
