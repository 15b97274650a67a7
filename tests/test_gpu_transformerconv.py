"""TransformerConv on the HIP path (csrc/edge_attention.hip) against the plain-torch restatement of
tests/transformerconv_oracle.py.

Tolerances are the project's own (tests/helpers.py), no new constants: the output and every gradient go through
``referee`` / ``referee_all`` -- |HIP - f64| <= 2 |oracle_f32 - f64| + 8 2^-23 max|f64|, the restatement's float32 and
float64 evaluations being the two oracles -- and through ``teeth``: the float64 run with the single edge removed that
changes the output most must be REJECTED by the same bar.

The operator is smooth (a softmax), so the operator cases carry no condition on their inputs.  The model cases have the
ReLUs between the layers, in the feed-forward blocks and in the heads: every ReLU input of the float64 run must lie
farther from zero than 4 x the referee's own limit for that tensor (``_check_gates``, no exclusion); the seeds were
chosen on the CPU, from the restatement alone, so that it holds.

One tensor per layer is zero in exact arithmetic whatever the graph: ``lin_key.bias``.  A shift of every key by the same
vector b moves all logits of a target i by q_i . b, which the softmax removes, so d lin_key.bias = sum_j dk_j = 0 and any
float32 evaluation holds rounding residue there.  The referee's scale max|grad| says nothing about such a sum; these
tensors -- named explicitly, with this reason -- may pass by the a-priori bound of ``TermMagnitudes`` instead
(``referee_all(cancelling=...)``), whose teeth are shown with the largest term of the sum removed (``bound_teeth``)."""
import copy

import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT, GPSConfig, HSCNConfig, MPNNConfig
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.model.hscn import HSCN, build_hscn
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import Relation
from tests import transformerconv_oracle as TO
from tests.helpers import DEV, KinkGuard, grads_of, hetero_batch, most_changed, referee_all, teeth

pytestmark = pytest.mark.gpu

LONG, CHUNK = Fh.EDGE_ATTN_LONG_ROW, Fh.EDGE_ATTN_CHUNK
NAMES = ("q", "k", "v", "e")
KEY_BIAS = ("zero in exact arithmetic: a shift of every key moves all logits of a target alike, which the softmax "
            "removes (module docstring)")


# --------------------------------------------------------------------------- #
# inputs and the two evaluations
# --------------------------------------------------------------------------- #
def _multigraph(N, E, seed):
    """The shape of tests/test_gpu_gine.py: [2, E] in RANDOM edge order (so that the CSR's eid[slot] != slot), the last
    four nodes isolated, nodes 1 and 2 with a self loop each, the first two random edges occurring three times."""
    g = torch.Generator().manual_seed(seed)
    live = max(N - 4, 1)
    base = torch.randint(0, live, (2, E - 6), generator=g)
    extra = torch.tensor([[1 % live, 2 % live], [1 % live, 2 % live]])
    ei = torch.cat([base, extra, base[:, :2], base[:, :2]], 1)
    return ei[:, torch.randperm(E, generator=g)].contiguous()


def _inputs(Ns, Nd, E, heads, C, seed, with_e=True):
    """(q [Nd, HC], k, v [Ns, HC], e [E, HC] or None), float32, standard normal (e with standard deviation 0.5)."""
    g = torch.Generator().manual_seed(1000 + seed)
    HC = heads * C
    return (torch.randn(Nd, HC, generator=g), torch.randn(Ns, HC, generator=g), torch.randn(Ns, HC, generator=g),
            0.5 * torch.randn(E, HC, generator=g) if with_e else None)


def _cotangent(Nd, HC, seed=7):
    return torch.randn(Nd, HC, generator=torch.Generator().manual_seed(seed))


def _oracle(t, ei, heads, gy, dtype, needs=NAMES, skip=None, e_rows=None):
    """{"out", "x.q", "x.k", "x.v", "x.e"}: the restatement in ``dtype``; ``e_rows``: the row of e each edge reads
    instead of its own (the wrong-row variant)."""
    leaves = {n: (None if x is None else x.detach().to(dtype).requires_grad_(n in needs)) for n, x in zip(NAMES, t)}
    e = leaves["e"] if e_rows is None else leaves["e"][e_rows]
    out = TO.aggregate(leaves["q"], leaves["k"], leaves["v"], e, ei, heads, skip)
    if out.requires_grad:
        out.backward(gy.to(dtype))
    res = {"out": out.detach()}
    res.update({"x." + n: x.grad for n, x in leaves.items() if x is not None})
    return res


def _hip(t, ei, heads, gy, needs=NAMES, rel=None, unaligned_q=False):
    Nd, Ns = t[0].size(0), t[1].size(0)
    rel = rel if rel is not None else Relation(ei.to(DEV), Ns, Nd)
    leaves = {n: (None if x is None else x.detach().to(DEV)) for n, x in zip(NAMES, t)}
    if unaligned_q:                                        # an offset-by-one-float view: contiguous, 4-byte aligned
        store = torch.empty(t[0].numel() + 1, dtype=torch.float32, device=DEV)
        leaves["q"] = store[1:].view_as(t[0]).copy_(leaves["q"])
        assert leaves["q"].data_ptr() % 16 == 4 and leaves["q"].is_contiguous()
    for n, x in leaves.items():
        if x is not None:
            x.requires_grad_(n in needs)
    out = Fh.EdgeAttentionFn.apply(leaves["q"], leaves["k"], leaves["v"], leaves["e"], rel, heads)
    if out.requires_grad:
        out.backward(gy.to(DEV))
    res = {"out": out.detach()}
    res.update({"x." + n: x.grad for n, x in leaves.items() if x is not None})
    return res, rel


def _check(what, t, ei, heads, needs=NAMES, with_teeth=True, **hip_kw):
    """Forward and every gradient under the referee, with its teeth; returns (HIP results, float32, float64)."""
    gy = _cotangent(t[0].size(0), t[0].size(1))
    o32, o64 = _oracle(t, ei, heads, gy, torch.float32, needs), _oracle(t, ei, heads, gy, torch.float64, needs)
    got, _ = _hip(t, ei, heads, gy, needs, **hip_kw)
    assert got["out"].shape == t[0].shape
    referee_all(got, o32, o64, what)
    if with_teeth and ei.size(1):
        t64 = [None if x is None else x.double() for x in t]
        d64 = _oracle(t, ei, heads, gy, torch.float64, needs, skip=TO.most_changing_edge(*t64, ei, heads))
        reached = most_changed(o64, [d64])
        alone = int(torch.bincount(ei[1]).max()) == 1       # one logit per softmax: q and k have zero gradients
        assert set(reached) == {k for k, v in o64.items() if v is not None and not (alone and k in ("x.q", "x.k"))}, \
            (what, sorted(reached))
        teeth(got, o32, o64, reached, what)
    return got, o32, o64


# --------------------------------------------------------------------------- #
# 1. the multigraph at every width class
# --------------------------------------------------------------------------- #
# the issue's widths, and the two at which a head takes a second column pass: (1, 512) with 16-byte accesses (64 lanes x
# 4 columns x 2), (2, 70) with 4-byte accesses (64 lanes x 2)
WIDTHS = [(1, 10), (1, 16), (2, 8), (3, 5), (4, 4), (4, 16), (8, 64), (1, 512), (2, 70)]


@pytest.mark.parametrize("with_e", [False, True], ids=["plain", "edge-features"])
@pytest.mark.parametrize("heads,C", WIDTHS)
def test_multigraph_under_the_float64_referee(heads, C, with_e):
    N, E = 37, 150
    ei = _multigraph(N, E, 3)
    order = torch.argsort(ei[1], stable=True)              # eid[slot] of the target-keyed stable CSR
    assert not torch.equal(order[:E], torch.arange(E))
    t = _inputs(N, N, E, heads, C, heads * 100 + C, with_e)
    what = f"edge attention multigraph heads={heads} C={C}" + (" with e" if with_e else "")
    got, o32, o64 = _check(what, t, ei, heads)
    iso = torch.bincount(ei[1], minlength=N) == 0
    assert int(iso.sum()) >= 4
    assert bool((got["out"].cpu()[iso] == 0).all()), "an isolated node's row is not exactly 0"
    assert bool((got["x.q"].cpu()[iso] == 0).all())
    if not with_e:
        assert "x.e" not in got
        return
    # the wrong row: e[slot] in place of e[eid[slot]], and de written in slot order -- the bar must see both
    slot_of_edge = torch.empty(E, dtype=torch.long)
    slot_of_edge[order] = torch.arange(E)
    gy = _cotangent(N, heads * C)
    wrong = _oracle(t, ei, heads, gy, torch.float64, e_rows=slot_of_edge)
    teeth(got, o32, o64, {"out": wrong["out"], "x.q": wrong["x.q"], "x.e": o64["x.e"][order]}, what + " [wrong row]")


# --------------------------------------------------------------------------- #
# 2. long rows: the threshold and the chunk edge, in both walks
# --------------------------------------------------------------------------- #
DEGREES = (LONG - 1, LONG, LONG + 1, LONG + CHUNK + 1)


def _long_rows(seed):
    """48 nodes: targets 0..3 with the in-degrees DEGREES (sources among 8..47), sources 4..7 with the same
    out-degrees (targets among 8..47), in random edge order."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for i, d in enumerate(DEGREES):
        others = torch.randint(8, 48, (d,), generator=g)
        parts.append(torch.stack([others, torch.full((d,), i)]))
        others = torch.randint(8, 48, (d,), generator=g)
        parts.append(torch.stack([torch.full((d,), 4 + i), others]))
    ei = torch.cat(parts, 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


@pytest.mark.parametrize("heads,C,with_e", [(2, 8, True), (1, 10, False), (3, 5, True), (4, 16, False)])
def test_long_rows_at_the_threshold_and_the_chunk_edge(heads, C, with_e):
    ei = _long_rows(5)
    assert tuple(torch.bincount(ei[1], minlength=48)[:4].tolist()) == DEGREES
    assert tuple(torch.bincount(ei[0], minlength=48)[4:8].tolist()) == DEGREES
    t = _inputs(48, 48, ei.size(1), heads, C, 11 + C, with_e)
    _check(f"edge attention long rows heads={heads} C={C}" + (" with e" if with_e else ""), t, ei, heads)


# --------------------------------------------------------------------------- #
# 3. bipartite relations, degenerate shapes
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_e", [False, True], ids=["plain", "edge-features"])
def test_bipartite_many_to_few(with_e):
    g = torch.Generator().manual_seed(2)
    ei = torch.stack([torch.randint(0, 50, (400,), generator=g), torch.randint(0, 4, (400,), generator=g)])
    _check("edge attention 50 -> 4" + (" with e" if with_e else ""), _inputs(50, 4, 400, 2, 8, 21, with_e), ei, 2)


@pytest.mark.parametrize("with_e", [False, True], ids=["plain", "edge-features"])
def test_bipartite_one_in_edge_per_target_is_a_copy(with_e):
    g = torch.Generator().manual_seed(4)
    ei = torch.stack([torch.randint(0, 4, (50,), generator=g), torch.randperm(50, generator=g)])
    t = _inputs(4, 50, 50, 2, 8, 22, with_e)
    got, _, _ = _check("edge attention 4 -> 50" + (" with e" if with_e else ""), t, ei, 2)
    want = torch.empty(50, 16)
    want[ei[1]] = t[2][ei[0]] + t[3] if with_e else t[2][ei[0]]
    assert torch.equal(got["out"].cpu(), want), "with one in-edge the weight is 1: out = v[j] (+ e) bit for bit"
    assert bool((got["x.q"].cpu() == 0).all())             # a softmax over one logit does not depend on it


def test_no_edges():
    t = _inputs(5, 7, 0, 2, 8, 23)
    ei = torch.zeros(2, 0, dtype=torch.int64)
    got, _, _ = _check("edge attention E = 0", t, ei, 2)
    assert bool((got["out"] == 0).all()) and got["x.e"].shape == (0, 16)
    for n in ("q", "k", "v"):
        assert bool((got["x." + n] == 0).all()), n         # exact zeros, not None


def test_the_last_rows_are_empty():
    g = torch.Generator().manual_seed(6)
    ei = torch.stack([torch.randint(0, 9, (40,), generator=g), torch.randint(0, 11, (40,), generator=g)])
    got, _, _ = _check("edge attention, last targets empty", _inputs(9, 13, 40, 3, 5, 24), ei, 3)
    assert bool((got["out"].cpu()[11:] == 0).all())


@pytest.mark.parametrize("heads,C", [(2, 8), (1, 128)])
def test_an_unaligned_view_of_q_takes_the_scalar_path(heads, C):
    ei = _multigraph(37, 150, 8)
    t = _inputs(37, 37, 150, heads, C, 25 + C)
    got, _, _ = _check(f"edge attention, q offset by one float, heads={heads} C={C}", t, ei, heads, unaligned_q=True)
    assert got["x.q"].data_ptr() % 16 == 0


# --------------------------------------------------------------------------- #
# 4. numerical stability, gradient patterns, reproducibility
# --------------------------------------------------------------------------- #
def test_large_logits_need_the_running_maximum():
    """Logits between about -100 and exactly +100: exp overflows float32 beyond 88.7 unless the running maximum is
    subtracted first."""
    heads, C = 2, 8
    ei = _multigraph(37, 150, 9)
    q, k, v, e = _inputs(37, 37, 150, heads, C, 26)
    s = ((q[ei[1]] * (k[ei[0]] + e)).view(-1, heads, C).sum(-1) / C ** 0.5).max()
    q = q * (100.0 / float(s))
    s = (q[ei[1]] * (k[ei[0]] + e)).view(-1, heads, C).sum(-1) / C ** 0.5
    assert 99.0 < float(s.max()) < 101.0 and float(s.min()) < -60.0
    assert not bool(torch.isfinite(torch.exp(s)).all())            # exp(100) is beyond float32
    got, _, _ = _check("edge attention, logits of magnitude 100", (q, k, v, e), ei, heads)
    assert all(bool(torch.isfinite(x).all()) for x in got.values())


@pytest.mark.parametrize("needs", [("q",), ("e",), ("k", "v"), ("v",)])
def test_gradient_patterns(needs):
    ei = _multigraph(37, 150, 10)
    t = _inputs(37, 37, 150, 2, 8, 27)
    got, _, o64 = _check(f"edge attention, gradients of {needs} only", t, ei, 2, needs=needs, with_teeth=False)
    for n in NAMES:
        assert (got["x." + n] is None) == (n not in needs) == (o64["x." + n] is None)


def test_an_output_without_cotangent_gives_none():
    ei = _multigraph(37, 150, 10).to(DEV)
    q, k, v, e = (x.to(DEV).requires_grad_(True) for x in _inputs(37, 37, 150, 2, 8, 27))
    out = Fh.EdgeAttentionFn.apply(q, k, v, e, Relation(ei, 37, 37), 2)
    (q.sum() + 0.0 * out.detach().sum()).backward()        # the operator's output is not on the path to the loss
    assert bool((q.grad == 1).all()) and k.grad is None and v.grad is None and e.grad is None
    # without edge features the fourth input has no gradient slot to fill
    q2 = q.detach().requires_grad_(True)
    Fh.EdgeAttentionFn.apply(q2, k.detach(), v.detach(), None, Relation(ei, 37, 37), 2).sum().backward()
    assert q2.grad is not None


def _graph(n, seed, long_target=False):
    ei = _multigraph(n, 4 * n, seed)
    if long_target:                                        # one row that the whole workgroup takes in chunks
        g = torch.Generator().manual_seed(seed)
        ei = torch.cat([ei, torch.stack([torch.randint(0, n, (LONG + 5,), generator=g), torch.zeros(LONG + 5, dtype=torch.long)])], 1)
    return ei


def test_two_runs_and_a_graph_alone_or_inside_a_batch_give_the_same_bits():
    heads, C = 4, 4
    sizes, seeds = (23, 31, 40), (1, 2, 3)
    eis = [_graph(n, s, long_target=(i == 1)) for i, (n, s) in enumerate(zip(sizes, seeds))]
    ts = [_inputs(n, n, ei.size(1), heads, C, 30 + i) for i, (n, ei) in enumerate(zip(sizes, eis))]
    gys = [_cotangent(n, heads * C, 40 + i) for i, n in enumerate(sizes)]
    alone, _ = _hip(ts[1], eis[1], heads, gys[1])
    again, _ = _hip(ts[1], eis[1], heads, gys[1])
    for key in alone:
        assert torch.equal(alone[key], again[key]), key
    off = np.cumsum([0] + list(sizes))
    ei = torch.cat([e + int(off[i]) for i, e in enumerate(eis)], 1)
    t = tuple(torch.cat([x[i] for x in ts], 0) for i in range(4))
    both, _ = _hip(t, ei, heads, torch.cat(gys, 0))
    lo, hi = int(off[1]), int(off[2])
    elo = eis[0].size(1)
    for key in alone:
        rows = slice(elo, elo + eis[1].size(1)) if key == "x.e" else slice(lo, hi)
        assert torch.equal(alone[key], both[key][rows]), f"{key}: a row depends on its place in the batch"


# --------------------------------------------------------------------------- #
# 5. models
# --------------------------------------------------------------------------- #
def _check_gates(g32, g64, what):
    """Every ReLU input of the float64 run farther from zero than 4 x the referee's own limit for its tensor."""
    assert set(g32) == set(g64) and g64
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"{what} {tag}")


def _twin(ref, call, gy, dtype, skip=None, chain_extra=None):
    """One evaluation of the restatement ``ref`` in ``dtype`` from a copy: ``call(model, dtype, skip)`` is its forward.
    Returns (parameter gradients, output, ReLU inputs seen, cotangents of every lin_key output, TermMagnitudes or None)."""
    from tests.test_gpu_attention import _Terms
    m = copy.deepcopy(ref).to(dtype)
    seen, cot, hooks = {}, {}, []
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    for name, mod in m.named_modules():
        if name.endswith("lin_key"):
            hooks.append(mod.register_forward_hook(
                lambda mod_, a, out, key=f"p.{name}.bias": out.register_hook(
                    lambda g: cot.__setitem__(key, g.detach().double().clone())) and None))
    tm = None
    if chain_extra is not None:
        tm = _Terms(m)
        tm.chain += chain_extra
    out = call(m, dtype, skip)
    out.backward(gy.to(dtype))
    for h in hooks:
        h.remove()
    if tm is not None:
        tm.close()
    g = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
    return g, out.detach(), seen, cot, tm


def _row_dropped(o64, key, cot):
    """``o64`` with the largest row removed from the bias gradient ``key`` = sum_r cot[r]: the toothed reference of a
    sum that is zero in exact arithmetic whatever the graph (no removed edge reaches it)."""
    d = dict(o64)
    d[key] = o64[key] - cot[int(cot.abs().max(1).values.argmax())]
    return d


def _model_check(what, ref, call, gy, skip, chain_extra, product, more_cancelling=(), more_skips=(), draws=()):
    """The whole model case: gates, forward and every parameter gradient under the referee, teeth.  ``product()``
    returns (model, prediction) after its backward.  ``more_cancelling``: further tensors of this case that may take the
    a-priori bound, with their reasons; ``more_skips``: further toothed variants of ``call`` that reach them.
    ``draws``: further float32 evaluations of the same function, each returning (gradients, prediction); the referee's
    yardstick is then the largest distance of a float32 draw (``helpers.referee``)."""
    o32, y32, g32, _, _ = _twin(ref, call, gy, torch.float32)
    if draws:
        more32 = [d() for d in draws]
        o32, y32 = [o32] + [d[0] for d in more32], [y32] + [d[1] for d in more32]
    o64, y64, g64, cot, terms = _twin(ref, call, gy, torch.float64, chain_extra=chain_extra)
    d64, dy64, _, _, _ = _twin(ref, call, gy, torch.float64, skip=skip)
    _check_gates(g32, g64, what)
    pm, pred, *layer_outputs = product()
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    if layer_outputs:                                      # tensors the prediction does not see, under the same names
        referee_all(layer_outputs[0], {k: g32[k] for k in layer_outputs[0]}, {k: g64[k] for k in layer_outputs[0]}, what)
    p32 = [{"pred": y} for y in y32] if isinstance(y32, list) else {"pred": y32}
    referee_all({"pred": pred}, p32, {"pred": y64}, what)
    teeth({"pred": pred}, p32, {"pred": y64}, {"pred": dy64}, what)
    got = grads_of(pm)
    assert set(got) == set(o64)
    # lin_key.bias of every layer that received a cotangent (HSCN's lv / vv relations do not reach the prediction)
    cancelling = {k: KEY_BIAS for k in cot if o64[k] is not None}
    assert cancelling
    cancelling.update(more_cancelling)
    referee_all(got, o32, o64, what, terms=terms, cancelling=list(cancelling))
    drops = [d64] + [_twin(ref, call, gy, torch.float64, skip=s)[0] for s in more_skips]
    drops += [_row_dropped(o64, k, cot[k]) for k in cot if o64[k] is not None]
    terms.bound_teeth(got, o32, o64, drops, list(cancelling), what)
    edge_reached = most_changed(o64, [d64])
    teeth(got, o32, o64, {k: v for k, v in edge_reached.items() if k not in cancelling}, what)
    return got, o64, edge_reached


def _layer0_edge(conv, x_src, x_dst, ei, edge_attr=None):
    """The edge whose removal changes the first layer's attention output most (float64)."""
    c = copy.deepcopy(conv).double()
    with torch.no_grad():
        e = c.lin_edge(edge_attr.double()) if c.lin_edge is not None else None
        return TO.most_changing_edge(c.lin_query(x_dst.double()), c.lin_key(x_src.double()), c.lin_value(x_src.double()),
                                     e, ei, c.heads)


def _pairs(b, seed):
    """Candidate pairs inside every graph of the batch (peptides graphs carry none of their own): [2, 64]."""
    g = torch.Generator().manual_seed(seed)
    ptr = b.ptr.tolist()
    return torch.cat([torch.randint(lo, hi, (2, 16), generator=g) for lo, hi in zip(ptr[:-1], ptr[1:])], 1)


# ---- the MPNN baseline ----------------------------------------------------------------------------------------------
# Eight float32 draws (tests/test_gpu_scn_resident_f64.py's count).  Peptides atom features reach 118, so the first layer's
# keys and queries reach 10^2 and its logits 10^3..10^4: rounding a logit to float32 alone moves an attention weight by
# 2^-24 |s| ~ 10^-4..10^-3 relative, in ANY float32 evaluation, and near a tie between two edges one evaluation's error
# says little about another's.  ``relabel_graphs`` would not redraw that error -- a logit is a sum over channels, not
# over nodes or edges -- so the further draws rearrange the channels instead (``_rearranged``): the same function in
# exact arithmetic, every Linear and every logit summed in another order.
DRAWS = 8


def _rearranged(ref, x, seed):
    """A copy of the ``MPNNRef`` ``ref`` computing the same function of ``x[:, cols]``: the input columns permuted
    (with the first layer's weight columns), and per layer the channels permuted within every head -- rows of lin_key /
    lin_query, and in a hidden layer also of lin_value / lin_skip / lin_edge together with the next layer's weight
    columns (the last layer keeps its output order; with edge features, which pair a key channel with a value channel,
    it keeps its key channels too).  Returns (model, x[:, cols], {parameter name: (row order, column order)})."""
    g = torch.Generator().manual_seed(seed)
    m = copy.deepcopy(ref)
    cols = torch.randperm(x.size(1), generator=g)
    x, order = x[:, cols], {}
    for li, c in enumerate(m.conv_layers):
        last = li == len(m.conv_layers) - 1
        rows = torch.cat([h * c.out_channels + torch.randperm(c.out_channels, generator=g) for h in range(c.heads)])
        if last and c.lin_edge is not None:
            rows = torch.arange(rows.numel())
        same = torch.arange(rows.numel())
        for name in ("lin_key", "lin_query", "lin_value", "lin_skip", "lin_edge"):
            lin = getattr(c, name)
            if lin is None:
                continue
            r = rows if (name in ("lin_key", "lin_query") or not last) else same
            cc = torch.arange(lin.in_features) if name == "lin_edge" else cols
            with torch.no_grad():
                lin.weight.copy_(lin.weight[r][:, cc])
                order[f"p.conv_layers.{li}.{name}.weight"] = (r, cc)
                if lin.bias is not None:
                    lin.bias.copy_(lin.bias[r])
                    order[f"p.conv_layers.{li}.{name}.bias"] = (r, None)
        cols = same if last else rows
    return m, x, order


def _restored(grads, order):
    """Parameter gradients of a ``_rearranged`` model in the original channel order."""
    out = {}
    for k, g in grads.items():
        if k in order and g is not None:
            r, c = order[k]
            back = torch.empty_like(g)
            if c is None:
                back[r] = g
            else:
                back[r.unsqueeze(1), c.unsqueeze(0)] = g
            g = back
        out[k] = g
    return out


# Seeds chosen on the CPU, from the restatement alone: the one of 0..7 (0..29 with the bond encoder) whose float64 run
# keeps its ReLU inputs farthest from zero in units of the required distance (17 x, 17 x, 17 x, 8.1 x, 3.3 x; about half
# of the seeds keep it at all -- 642 nodes x 16 channels x 2 layers of values spread over +-30).
MPNN_H, MPNN_L, MPNN_HEADS = 16, 3, 4
MPNN_CASES = {          # conv_type, task level, edge features, edge encoder, width of the last layer, seed
    "graph": ("transformerconv", "graph", False, None, 10, 5),
    "node": ("transformerconv", "node", False, None, 10, 5),
    "link": ("transformerconv", "link", False, None, 8, 5),
    "edge": ("transformerconv_edge", "graph", True, None, 10, 7),
    "edge-bond": ("transformerconv_edge", "graph", True, "bond", 10, 25),
}


def _mpnn_reference(case):
    """Everything of a model case that is computed on the CPU (the seed search runs this alone)."""
    from graph_hscn.encoder.categorical import BOND_FEATURE_DIMS
    conv, level, edges, enc, C, seed = MPNN_CASES[case]
    graphs = make_dataset("peptides_func", 4, seed=seed, edge_features=edges)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(seed)
    ref = TO.MPNNRef(9, MPNN_H, C, MPNN_L, MPNN_HEADS, int(b.edge_attr.size(1)) if edges and enc is None else None,
                     level, BOND_FEATURE_DIMS if enc else None)
    pairs = _pairs(b, seed) if level == "link" else None
    rows = {"graph": (int(b.num_graphs), C), "node": (int(b.num_nodes), C)}.get(level) or (int(pairs.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))
    x = b.x.float()

    def call(m, dtype, skip, x=x):
        ea = None if not edges else (b.edge_attr if enc else b.edge_attr.to(dtype))
        return m(x.to(dtype), b.edge_index, ea, b.batch, int(b.num_graphs), pairs, skip)

    def draw(r):
        m, xr, order = _rearranged(ref, x, 100 * seed + r)
        g, y, _, _, _ = _twin(m, lambda mm, dtype, skip: call(mm, dtype, skip, xr), gy, torch.float32)
        return _restored(g, order), y
    draws = [lambda r=r: draw(r) for r in range(1, DRAWS)]

    with torch.no_grad():
        ea0 = None if not edges else (ref.edge_encoder(b.edge_attr) if enc else b.edge_attr.float())
    skip = _layer0_edge(ref.conv_layers[0], x, x, b.edge_index, ea0)
    # what TermMagnitudes does not count itself: per layer the softmax and the sum over the largest in-degree (+ 8);
    # the pool's segment
    chain = MPNN_L * (int(torch.bincount(b.edge_index[1]).max()) + 8) + int(torch.bincount(b.batch).max())
    return ref, b, pairs, gy, call, skip, chain, draws


@pytest.mark.parametrize("case", list(MPNN_CASES))
def test_mpnn_under_the_float64_referee(case):
    from graph_hscn.train import batching
    conv, level, edges, enc, C, seed = MPNN_CASES[case]
    what = f"MPNN {conv} {level} level" + (" + BondEncoder" if enc else "")
    ref, b, pairs, gy, call, skip, chain, draws = _mpnn_reference(case)

    def product():
        pm = MPNN(CONV_DICT[conv], ACT_DICT["relu"], 9, MPNN_H, C, MPNN_L, dropout=0.0, task_level=level,
                  edge_encoder=enc, heads=MPNN_HEADS).to(DEV)
        if pairs is not None:
            b.edge_label_index = pairs
        bd = batching.to_device(pm, b, DEV)
        pm.engine = "auto"                                 # runs layered: the model has no resident form
        if edges:
            with torch.no_grad():
                pm(bd)                                     # edge_dim = -1: every lin_edge is sized by its first call
        pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
        pred = pm(bd)
        pred.backward(gy.to(DEV))
        pm.check_flags()
        return pm, pred

    got, o64, reached = _model_check(what, ref, call, gy, skip, chain, product, draws=draws)
    assert all(v is not None for v in got.values())
    assert len(got) == MPNN_L * (8 + (1 if edges else 0)) + (1 if enc else 0)
    assert {"p.conv_layers.0.lin_value.weight", "p.conv_layers.0.lin_query.weight", "p.conv_layers.1.lin_key.weight"} \
        <= set(reached), sorted(reached)
    if edges:
        assert "p.conv_layers.0.lin_edge.weight" in reached
    if enc:
        assert "p.edge_encoder.weight" in reached          # exists only because edge_attr carries a gradient


# ---- GPS with the attention local branch ---------------------------------------------------------------------------
GPS_D, GPS_HEADS, GPS_L, GPS_SEED = 16, 4, 2, 4          # of the seeds 0..7 the widest gate margin (17 x)


def _gps_reference():
    graphs = make_dataset("peptides_func", 4, seed=GPS_SEED, edge_features=True)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(GPS_SEED)
    ref = TO.gps_twin(9, GPS_D, 10, GPS_L, GPS_HEADS, int(b.edge_attr.size(1)))
    gy = torch.randn(int(b.num_graphs), 10, generator=torch.Generator().manual_seed(1))
    x, ea = b.x.float(), b.edge_attr.float()

    def call(m, dtype, skip):
        """``skip``: an edge number (left out of every layer's local attention), ("att", (g, j)): key j of graph g left
        out of the global attention, or ("pool", node): a node left out of the mean pool's sum."""
        kind, which = skip if isinstance(skip, tuple) else ("edge", skip)
        for layer in m.layers:
            layer.edge_skip = which if kind == "edge" else None
        return m(x.to(dtype), b.edge_index, ea.to(dtype), b.batch, b.ptr, int(b.num_graphs), None,
                 which if kind == "att" else None, which if kind == "pool" else None)

    with torch.no_grad():
        x0 = ref.node_encoder(x)
    skip = _layer0_edge(ref.layers[0].conv, x0, x0, b.edge_index, ea)
    chain = GPS_L * (int(torch.bincount(b.edge_index[1]).max()) + 8) + int(torch.bincount(b.batch).max())
    return ref, b, gy, call, skip, chain


def test_gps_with_the_attention_local_branch_under_the_float64_referee():
    from graph_hscn.train import batching
    what = "GPS local_conv=transformerconv_edge, graph level"
    ref, b, gy, call, skip, chain = _gps_reference()

    def product():
        pm = GPS(9, GPS_D, 10, GPS_L, num_heads=GPS_HEADS, local_conv="transformerconv_edge",
                 activation=ACT_DICT["relu"], dropout=0.0, norm="layer").to(DEV)
        bd = batching.to_device(pm, b, DEV)
        with torch.no_grad():
            pm(bd)
        pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
        pred = pm(bd)
        pred.backward(gy.to(DEV))
        pm.check_flags()
        return pm, pred

    more = {f"p.layers.{i}.attn.in_proj_bias": "the K third is zero in exact arithmetic (tests/test_gpu_attention.py)"
            for i in range(GPS_L)}
    more[f"p.layers.{GPS_L - 1}.norm2.bias"] = "equal parts of differing sign behind the mean pool (test_gpu_attention.py)"
    got, o64, reached = _model_check(what, ref, call, gy, skip, chain, product, more, [("att", (0, 0)), ("pool", 0)])
    assert all(v is not None for v in got.values())
    assert {"p.node_encoder.weight", "p.layers.0.conv.lin_edge.weight", "p.layers.0.conv.lin_value.weight",
            "p.lin_2.weight"} <= set(reached), sorted(reached)


# ---- HSCN with attention on all three relations ---------------------------------------------------------------------
HSCN_H, HSCN_L, HSCN_HEADS, HSCN_K, HSCN_SEED = 16, 2, 2, 4, 5      # of the seeds 0..7 the widest gate margin (6.6 x)


class _HB(dict):
    """The minimum of a batch ``HSCN._forward_layered`` reads (tests/test_gpu_layered_f64.py)."""

    def __init__(self, batch_local, num_graphs):
        super().__init__()
        self.num_graphs = num_graphs

        class L:
            batch = batch_local
        self["local"] = L()


def _hscn_reference():
    b, _ = hetero_batch("peptides_func", 4, HSCN_K, HSCN_SEED)
    torch.manual_seed(HSCN_SEED)
    ref = TO.HSCNRef(9, HSCN_H, 10, HSCN_L, HSCN_HEADS)
    gy = torch.randn(4, 10, generator=torch.Generator().manual_seed(1))
    xl, xv = b["x_dict"]["local"], b["x_dict"]["virtual"]

    def call(m, dtype, skip):
        return m({"local": xl.to(dtype), "virtual": xv.to(dtype)}, b["edge_index_dict"], b["batch_local"], 4, skip)

    ll = b["edge_index_dict"][TO.LL]
    skip = (TO.LL, _layer0_edge(ref.convs[0].convs["__".join(TO.LL)], xl, xl, ll))
    longest = max(int(torch.bincount(ei[1]).max()) for ei in b["edge_index_dict"].values())
    chain = HSCN_L * (longest + 8) + int(torch.bincount(b["batch_local"]).max())
    return ref, b, gy, call, skip, chain


def test_hscn_with_attention_on_every_relation_under_the_float64_referee():
    what = "HSCN TransformerConv x 3, heads=2"
    ref, b, gy, call, skip, chain = _hscn_reference()

    def product():
        pm = HSCN("TransformerConv", "TransformerConv", "TransformerConv", ACT_DICT["relu"], 9, HSCN_H, 10, HSCN_L,
                  heads=HSCN_HEADS).to(DEV)
        pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
        x = {k: v.to(DEV) for k, v in b["x_dict"].items()}
        eis = {k: v.to(DEV) for k, v in b["edge_index_dict"].items()}
        # without a virtual -> local relation the virtual branch never reaches the prediction: every layer's outputs of
        # both node types (the hard ReLU's inputs) are kept and checked by themselves
        layers = {}
        hooks = [conv.register_forward_hook(lambda m, a, out, li=li: layers.update(
            {f"layer {li} {k}": v.detach() for k, v in out.items()})) for li, conv in enumerate(pm.convs)]
        pred = pm(x, eis, _HB(b["batch_local"].to(DEV), 4))       # engine "auto": the relations are not the resident ones
        for h in hooks:
            h.remove()
        pred.backward(gy.to(DEV))
        assert set(layers) == {f"layer {li} {k}" for li in range(HSCN_L) for k in ("local", "virtual")}
        return pm, pred, layers

    got, o64, reached = _model_check(what, ref, call, gy, skip, chain, product)
    # the lv and vv relations feed the virtual nodes only: no gradient, None on both sides
    none = {k for k, v in o64.items() if v is None}
    assert none == {f"p.convs.{li}.convs.{r}.{p}" for li in range(HSCN_L)
                    for r in ("local__to__virtual", "virtual__to__virtual")
                    for p in ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias",
                              "lin_value.weight", "lin_value.bias", "lin_skip.weight", "lin_skip.bias")}
    assert {"p.convs.0.convs.local__to__local.lin_value.weight", "p.convs.1.convs.local__to__local.lin_query.weight"} \
        <= set(reached), sorted(reached)


# ---- two steps through the training loop ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["mpnn", "mpnn-edge-bond", "gps", "hscn"])
def test_two_training_steps_run_layered_with_a_finite_loss(model):
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.train import batching
    from graph_hscn.train.train import train_epoch
    graphs = make_dataset("peptides_func", 4, seed=1, edge_features=model in ("mpnn-edge-bond", "gps"))
    torch.manual_seed(1)
    if model == "hscn":
        rng = np.random.default_rng(1)
        batch = HeteroBatch.from_data_list([hetero_from_clusters(g, rng.integers(0, HSCN_K, g.num_nodes), HSCN_K)
                                            for g in graphs])
        pm = build_hscn(HSCNConfig("relu", "TransformerConv", "TransformerConv", "TransformerConv",
                                   hidden_channels=HSCN_H, num_layers=HSCN_L, heads=HSCN_HEADS), 9, 10).to(DEV)
    else:
        batch = Batch.from_data_list(graphs)
        if model == "gps":
            pm = build_gps(GPSConfig("relu", local_conv_type="transformerconv_edge", hidden_channels=GPS_D,
                                     num_layers=GPS_L, num_heads=GPS_HEADS, dropout=0.1), 9, 10).to(DEV)
        else:
            edge = model == "mpnn-edge-bond"
            pm = build_mpnn(MPNNConfig("transformerconv_edge" if edge else "transformerconv", "relu",
                                       hidden_channels=MPNN_H, num_layers=MPNN_L, dropout=0.1,
                                       edge_encoder="bond" if edge else None, heads=MPNN_HEADS), 9, 10).to(DEV)
        pm.engine = "auto"
        with torch.no_grad():
            pm(batching.to_device(pm, batch, DEV))         # sizes every lin_edge before the optimizer sees them
    opt = torch.optim.Adam(pm.parameters(), lr=1e-3)
    loss = train_epoch(0, None, [batch, batch], pm, opt, "cross_entropy", None, 1, False)[0]
    assert np.isfinite(loss)
    assert pm.last_engine == "layered"
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in pm.parameters())


def test_resident_entry_points_refuse_the_model_by_name_on_the_device():
    from types import SimpleNamespace

    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    graphs = make_dataset("peptides_func", 4, seed=0)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(0)
    pm = MPNN(CONV_DICT["transformerconv"], ACT_DICT["relu"], 9, 16, 10, 3, dropout=0.0, heads=4).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(bd)
    assert pm.last_engine == "layered" and out.shape == (4, 10)
    pm.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="convolution TransformerConv"):
        pm(bd)
    pm.engine = "layered"
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        MPNNResidentTrainStep(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        batching.resident_step(pm, bd, "cross_entropy")            # what replay.CapturedStep builds its step with
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        DeviceEvaluator(graphs, pm, "cross_entropy", 4).run()
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        fit_resident(None, opt, cfg, graphs, [], pm, 4)
