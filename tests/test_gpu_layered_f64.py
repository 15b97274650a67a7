"""The per-operator ("layered") engine THROUGH AUTOGRAD against a float64 referee: ``nn/functional.py``'s Functions,
the modules of ``nn/conv.py`` / ``nn/pool.py`` / ``nn/norm.py`` and the ``_forward_layered`` paths of ``model/hscn.py``
and ``model/mpnn.py`` -- which CSR side a backward walks, which weight permutation it uses, which
``needs_input_grad`` branch it takes, how ``HeteroConv`` sums.  (The kernels below them have their own float64 bounds
in tests/test_gpu_ops_f64.py.)

Every case is evaluated three times from identical weights and inputs: by the CPU oracle in float32, by
``copy.deepcopy(oracle).double()`` in float64, and by the HIP path.  The forward is held to the bar the suite already
uses for that operator (north_star's 1e-5; 2e-5 where a GAT softmax or a norm layer is involved, as in test_gpu_ops.py /
test_gpu_mpnn.py).  Every gradient -- inputs and parameters -- goes through ``helpers.referee``:

    |HIP - f64|  <=  2 |oracle_f32 - f64| + 8 * 2^-23 * max|f64|          (per tensor, max norm)

with the same ``None`` pattern as the oracle.  No tolerance here is measured from the code under test.

Teeth (operator cases): a second float64 reference with ONE term removed -- one edge of the graph, one row of the
pooled segment, one row of a linear layer's batch -- must be REJECTED by the same referee, for every gradient that term
reaches.  Per gradient tensor the candidate whose removal changes that tensor most is used; the candidates are all
edges of a small graph, else a fixed sample of 48 (the hub's edges among them) -- the largest change over a sample is no
larger than over all edges, so sampling only makes rejection harder.  A tensor that does not depend on the term at
all (a GCNConv bias gradient is a column sum of the cotangent) is equal in both float64 evaluations and is skipped.

Kink guard: ReLU and the GAT leaky-ReLU make a gradient discontinuous in the forward values.  ``helpers.KinkGuard``
records, from the float64 oracle alone, every ReLU input and every attention logit and asserts each is farther from
zero than 4 x the forward bar this file asserts; the forward check comes first, so no gate can differ between the three
evaluations.  The committed seeds were chosen on the CPU so that the oracle satisfies it; the assertion stays so that a
change of seed or shape cannot silently void the referee.  (ELU's derivative is continuous at 0, tanh is smooth.)

Where the referee's scale says nothing (model cases).  The referee measures against max|grad|.  A parameter gradient is
a sum over rows (nodes) of cotangent row x input row, and some of these sums cancel by construction: a convolution bias
in front of a BatchNorm has a zero gradient in exact arithmetic, ``att_dst`` shifts every logit of a target alike (the
softmax removes it except across the leaky kink), a first-layer bias sums cotangents of both signs.  Their float32
values carry rounding residue ~ rows * 2^-24 * sum|terms| in ANY evaluation order, while max|grad| is far smaller; and
the CPU oracle's pairwise sums make |oracle32 - f64| small.  On the MI355X the referee rejected, with its three numbers
(|HIP - f64|, |oracle32 - f64|, ulp of the scale) and ratio, for example
    HSCN GAT/GCN/GCN L=2 H=16  convs.0 ll bias       1.395e-07  1.474e-08  9.367e-09   1.336
    HSCN GAT/GAT/GAT L=2 H=16  convs.1 ll att_dst    4.029e-07  5.830e-08  7.244e-09   2.308
    MPNN gat plain             conv_layers.0 att_dst 1.804e-05  2.064e-06  2.030e-07   3.136
    MPNN gcn bn+ln             conv_layers.0 bias    9.030e-07  1.258e-07  1.634e-08   2.361
    SCN dense-ragged K=4 relu  mp.module_0 lin_rel.W 4.459e-09  9.019e-10  3.156e-11   2.168
(the full list is in profiles/layered_f64_referee.txt; every operator case of section B passes the referee itself).
None is a kernel fault: against sum|terms| the same errors are 1e-7 .. 1e-5 relative.  These (case, tensor) pairs, and
no others, are listed in CANCELLING below with the reason their sum cancels; a listed tensor that the referee rejects is
held to the a-priori ``f64_close`` form instead, |got - f64| <= 3 n 2^-24 mag, with ``mag`` = the sum of |cotangent row|
x |input row| recorded from the float64 oracle and n = rows + the lengths of the sums on the paths through that
parameter (``helpers.TermMagnitudes`` has the derivation and its limits; nothing in it is measured from the code under
test).  Every tensor that is not listed passes the referee or the test fails.  The bound has to show its teeth in every
case that may use it: a float64 reference with one edge removed (the one that changes the tensor most, among up to 48)
must be rejected by the referee AND by the bound.

Each test prints its referee lines and the worst ratio |HIP - f64| / limit; profiles/layered_f64_referee.txt records one
run of them.  Nothing is asserted from that file.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import models as OM
from oracle import pyg_ops as P
from tests.helpers import (ATOL, DEV, RTOL, close, grads_of, most_changed, oracle_twin, referee, referee_all,
                           scn_step_in_dtype, teeth)

pytestmark = pytest.mark.gpu

MAX_CANDIDATES = 48


# --------------------------------------------------------------------------- #
# the three evaluations
# --------------------------------------------------------------------------- #
def _cast(v, dtype, dev=None):
    if isinstance(v, torch.Tensor):
        if v.is_floating_point():
            v = v.to(dtype)
        return v.to(dev) if dev is not None else v
    if isinstance(v, (list, tuple)):
        return type(v)(_cast(t, dtype, dev) for t in v)
    if isinstance(v, dict):
        return {k: _cast(t, dtype, dev) for k, t in v.items()}
    return v


def _oracle_eval(om, x, consts, gy, dtype, gates=None, steps=1, chain_extra=None, guard=False):
    """``om(**x, **consts)`` and its backward under the cotangent ``gy`` in ``dtype``, through ``helpers.oracle_twin``.
    Returns (out, gradients, kink guard or None, TermMagnitudes or None)."""
    keep = {}

    def step(m, dt):
        xs = {k: v.detach().clone().to(dt).requires_grad_() for k, v in x.items()}
        keep["out"] = m(**xs, **_cast(consts, dt))
        keep["out"].backward(gy.to(dt))
        return {k: v.grad for k, v in xs.items()}

    grads, kg, terms = oracle_twin(om, step, dtype, gates, chain_extra, steps, guard)
    return keep["out"].detach(), grads, kg, terms


def _product_eval(pm, x, consts, gy, steps=1):
    out = grads = None
    dconsts = _cast(consts, torch.float32, DEV)
    for _ in range(steps):
        pm.zero_grad(set_to_none=True)
        xs = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in x.items()}
        out = pm(**xs, **dconsts)
        out.backward(gy.to(DEV))
        torch.cuda.synchronize()
        grads = grads_of(pm, **xs)
    return out.detach(), grads


# The (case, tensor) pairs that may pass by helpers.TermMagnitudes' a-priori bound where the referee rejects them, each
# with the reason its sum cancels.  Every other tensor of every case passes the referee or the test fails; for the
# tensors listed, a reference with one edge removed must be rejected by referee and bound together (bound_teeth).
_NORM = "in front of a BatchNorm, which removes a column's shift and scale: the cotangent columns sum to ~0"
_ATT = "attention vector: a per-target shift of the logits, which the softmax removes except across the leaky kink"
_BIAS = "a column sum of cotangents of both signs over all nodes"
_MINCUT = "MinCUT losses are ratios invariant to the assignment's scale; softmax cotangent rows sum to zero"
_HL = "p.m.convs.%d.convs.local__to__local.%s"
CANCELLING = {
    "HSCN GAT/GCN/GCN L=2 H=16": {_HL % (0, "bias"): _BIAS, _HL % (1, "bias"): _BIAS},
    "HSCN GAT/GAT/GAT L=2 H=16": {_HL % (1, "att_dst"): _ATT},
    "HSCN GAT/GCN/GCN H=8 (layered only)": {_HL % (1, "bias"): _BIAS},
    "SCN dense K=4 sizes=(130,) adj=None directed=True mp_units=[16, 16] relu":
        {"p.m.mlp.0.weight": _MINCUT, "p.m.mlp.0.bias": _MINCUT},
    "SCN dense-ragged K=4 sizes=(64, 65, 2) adj=u8 directed=False mp_units=[16, 16] relu":
        {"p.m.mp.module_0.lin_rel.weight": _MINCUT, "p.m.mp.module_0.lin_rel.bias": _MINCUT,
         "p.m.mp.module_0.lin_root.weight": _MINCUT, "p.m.mp.module_2.lin_rel.weight": _MINCUT},
    "MPNN gat plain": {"p.m.conv_layers.0.att_dst": _ATT, "p.m.conv_layers.2.att_src": _ATT},
    "MPNN gcn bn+ln": {"p.m.conv_layers.0.bias": _NORM, "p.m.conv_layers.0.lin.weight": _NORM},
    "MPNN gat bn+ln": {"p.m.lns.0.bias": _BIAS, "p.m.conv_layers.0.att_dst": _ATT, "p.m.conv_layers.1.bias": _BIAS},
    "MPNN gat dropout": {"p.m.conv_layers.2.att_dst": _ATT},
}


def _references(what, om, x, consts, gy, gates=None, atol=ATOL, rtol=RTOL, drops=None, steps=1, chain_extra=0,
                draws=None):
    """The CPU side of ``_check``, which needs no device and which several engines on the same inputs can share: the
    float32 and float64 oracle evaluations, the kink guard on the float64 one (asserted here), the float64 evaluations
    of ``drops``.  ``draws``: further ``consts`` dicts that describe the SAME inputs (``helpers.relabel_graphs``); the
    float32 oracle is evaluated on each and the referee's yardstick becomes the largest distance over all of them
    (``helpers.referee``); gradients only -- the forward value is the one of ``consts``."""
    cancelling = CANCELLING.get(what, {})
    assert not cancelling or drops, f"{what}: tensors that may take the derived bound need its teeth"
    o32, g32, _, _ = _oracle_eval(om, x, consts, gy, torch.float32, steps=steps)
    o64, g64, kg, terms = _oracle_eval(om, x, consts, gy, torch.float64, gates, steps, chain_extra, guard=True)
    kg.check(atol, rtol, what)
    if draws:
        g32 = [g32] + [_oracle_eval(om, x, dc, gy, torch.float32, steps=steps)[1] for dc in draws]
    dropped = []
    for d in drops or []:
        dc, dg = d if isinstance(d, tuple) else (d, gy)
        dropped.append(_oracle_eval(om, x, dc, dg, torch.float64, steps=steps)[1])
    return dict(o32=o32, g32=g32, o64=o64, g64=g64, terms=terms, dropped=dropped, cancelling=cancelling)


def _judge(what, ref, od, gd, atol=ATOL, rtol=RTOL):
    """One engine's forward value ``od`` and gradients ``gd`` against the ``_references`` of the case: forward at
    (atol, rtol), every gradient through the referee, then the teeth.  Returns the worst ratio."""
    g32, g64, terms, cancelling, dropped = ref["g32"], ref["g64"], ref["terms"], ref["cancelling"], ref["dropped"]
    assert close(od, ref["o32"], atol=atol, rtol=rtol), f"{what}: forward outside the bar"
    worst = referee_all(gd, g32, g64, what, terms=terms, cancelling=cancelling)
    if dropped:
        if cancelling:
            terms.bound_teeth(gd, g32, g64, dropped, list(cancelling), what)
        else:
            reached = most_changed(g64, dropped)
            assert reached, f"{what}: the dropped term reaches no gradient"
            print(f"   teeth: one dropped term reaches {sorted(reached)}; untouched: {sorted(set(g64) - set(reached))}")
            teeth(gd, g32, g64, reached, what)
    return worst


def _check(what, om, pm, x, consts, gy, gates=None, atol=ATOL, rtol=RTOL, drops=None, steps=1, chain_extra=0,
           draws=None):
    """Forward at (atol, rtol) against the float32 oracle, kink guard on the float64 oracle, every gradient through
    the referee.  ``drops``: references with one term removed, each a ``consts`` dict or ``(consts, gy)``.  A case
    without an entry in CANCELLING: every tensor passes the referee, and the HIP result is rejected against the dropped
    reference for every gradient the term reaches (``teeth``).  A case listed there: its named tensors may take the
    derived bound, and referee and bound together must reject the dropped reference for them (``bound_teeth``).
    ``draws``: relabelled copies of the inputs for a yardstick over several float32 draws (``_references``); without
    them the single evaluation is the yardstick, as before."""
    print(f"[layered f64] {what}")
    ref = _references(what, om, x, consts, gy, gates, atol, rtol, drops, steps, chain_extra, draws)
    od, gd = _product_eval(pm, x, consts, gy, steps=steps)
    worst = _judge(what, ref, od, gd, atol, rtol)
    g32 = ref["g32"][0] if draws else ref["g32"]
    return worst, (ref["o32"], g32, ref["o64"], ref["g64"], od, gd)


def _drop_edges(ei, extra=(), must=()):
    """Edge lists with one edge removed: every edge when there are at most MAX_CANDIDATES, else an evenly spaced
    sample plus ``must`` (edge positions, e.g. the hub's first edges).  ``extra``: per-edge tensors cut alongside."""
    E = ei.size(1)
    if E == 0:
        return []
    if E <= MAX_CANDIDATES:
        idx = list(range(E))
    else:
        idx = sorted(set(torch.linspace(0, E - 1, MAX_CANDIDATES - len(must)).long().tolist()) | set(must))
    out = []
    for e in idx:
        keep = torch.ones(E, dtype=torch.bool)
        keep[e] = False
        out.append((ei[:, keep].contiguous(),) + tuple(t[keep].contiguous() for t in extra))
    return out


def multigraph(n, seed, hub=70, loops=True):
    """A DIRECTED multigraph on n nodes: ~3 random edges per node among the first ~90% (the rest are isolated), most
    (i -> j) without a (j -> i); five edges repeated (one of them three times); input self loops, one node with two;
    node 0 a hub of in-degree > 64 (``hub`` extra edges into it, sources repeating when n is small); edge order
    shuffled.  n = 1: the one node and, with ``loops``, its loop twice."""
    g = torch.Generator().manual_seed(seed)
    if n == 1:
        return torch.zeros(2, 2 if loops else 0, dtype=torch.long)
    m = max(2, n - max(1, n // 10))
    e = 3 * m
    src, dst = torch.randint(0, m, (e,), generator=g), torch.randint(0, m, (e,), generator=g)
    keep = src != dst
    ei = torch.stack([src[keep], dst[keep]])
    rep = ei[:, :5]
    parts = [ei, rep, rep[:, :1]]
    if hub:
        parts.append(torch.stack([torch.randint(1, m, (hub,), generator=g), torch.zeros(hub, dtype=torch.long)]))
    if loops:
        parts.append(torch.tensor([[1, 1, min(3, m - 1)], [1, 1, min(3, m - 1)]]))
    ei = torch.cat(parts, 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


def _hub_edges(ei, k=4):
    return torch.nonzero(ei[1] == 0).flatten()[:k].tolist()


def _randomise_biases(m, seed, std=0.3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * std)
    return m


# --------------------------------------------------------------------------- #
# B. operators.  Oracle and product wrappers share the call ``m(**inputs, **consts)`` and their parameter names; a
# ReLU's input passes through the oracle wrapper's ``gate`` (an Identity the kink guard hooks).
# --------------------------------------------------------------------------- #
class _OOp(nn.Module):
    def __init__(self, op, act="identity"):
        super().__init__()
        self.op, self.act, self.gate = op, act, nn.Identity()

    def _act(self, y):
        return OM.ACT[self.act](self.gate(y) if self.act == "relu" else y)


def _gate(m):
    return [m.gate] if m.act == "relu" else []


class OLinear(_OOp):
    def forward(self, x):
        return self._act(self.op(x))


class PLinear(nn.Module):
    def __init__(self, i, o, act, bias=True):
        super().__init__()
        from graph_hscn.nn import Linear
        self.op, self.act = Linear(i, o, bias=bias), act

    def forward(self, x):
        return self.op(x, act=self.act)


class OConv(_OOp):
    """``act(op(x, edge_index[, edge_weight]))``"""

    def forward(self, x, ei, ew=None):
        return self._act(self.op(x, ei) if ew is None else self.op(x, ei, ew))


class PConv(nn.Module):
    def __init__(self, op, act="identity"):
        super().__init__()
        self.op, self.act = op, act

    def forward(self, x, ei, ew=None):
        return self.op(x, ei, act=self.act) if ew is None else self.op(x, ei, ew, act=self.act)


def _load(pm, om):
    pm = pm.to(DEV)
    assert sorted(pm.state_dict()) == sorted(om.state_dict())
    pm.load_state_dict(om.state_dict())
    return pm


@pytest.mark.parametrize("act", ["identity", "relu", "elu", "tanh"])
@pytest.mark.parametrize("rows,i,o", [(1, 9, 16), (257, 32, 12), (64, 128, 128), (5, 16, 1)])
def test_linear(rows, i, o, act):
    g = torch.Generator().manual_seed(rows)
    torch.manual_seed(rows)
    om = _randomise_biases(OLinear(P.PygLinear(i, o), act), rows)
    pm = _load(PLinear(i, o, act), om)
    x = torch.randn(rows, i, generator=g)
    gy = torch.randn(rows, o, generator=g)
    # one term = one row of the batch: its cotangent removed (W, b lose that row's term, x loses that row)
    drops = []
    for r in sorted(set(torch.linspace(0, rows - 1, min(rows, 8)).long().tolist())):
        z = gy.clone()
        z[r] = 0
        drops.append(({}, z))
    _check(f"linear {rows}x{i}->{o} {act}", om, pm, {"x": x}, {}, gy, gates=_gate, drops=drops)


def _x(n, f, seed):
    return torch.randn(n, f, generator=torch.Generator().manual_seed(1000 + seed))


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("h", [10, 16, 32, 128])
@pytest.mark.parametrize("n", [1, 40, 300])
def test_gcn_conv(n, h, loops):
    from graph_hscn.nn import GCNConv
    fin, seed = 9, n + h
    ei = multigraph(n, seed)
    torch.manual_seed(seed)
    om = _randomise_biases(OConv(P.GCNConv(fin, h, add_self_loops=loops)), seed)
    pm = _load(PConv(GCNConv(fin, h, add_self_loops=loops)), om)
    gy = _x(n, h, seed + 1)
    drops = [{"ei": e} for (e,) in _drop_edges(ei, must=_hub_edges(ei))]
    if n == 1:
        drops = []            # the one node's two loops: normalised they sum to one edge's worth (or are replaced by the
        #                       appended loop), so removing one changes nothing: no teeth at n = 1
    _check(f"GCNConv n={n} H={h} add_self_loops={loops}", om, pm, {"x": _x(n, fin, seed)}, {"ei": ei}, gy, drops=drops)


def _graphconv_weights(kind, ei, n, seed):
    if kind == "unit":
        return ei, None
    if kind == "asym":                       # w_ij != w_ji wherever both directions exist: every edge its own draw
        return ei, torch.rand(ei.size(1), generator=torch.Generator().manual_seed(seed)) + 0.25
    return P.gcn_norm(ei, None, n, add_self_loops=True)       # "gcn_norm": the directed graph's normalised weights


@pytest.mark.parametrize("act", ["identity", "relu", "elu", "tanh"])
@pytest.mark.parametrize("kind", ["unit", "asym", "gcn_norm"])
def test_graph_conv_directed(kind, act):
    """The weighted GraphConv backward on a DIRECTED multigraph with asymmetric weights: ``gx`` walks ``rel.csr_t``
    with the weights permuted through ``csr_t.eid``; on a symmetric matrix (tests/test_gpu_ops.py) a walk over the wrong
    side or with the wrong permutation gives the same answer, here it does not."""
    from graph_hscn.nn import GraphConv
    n, fin, h, seed = 150, 9, 16, 7
    ei0 = multigraph(n, seed)
    rev = set(map(tuple, ei0.flip(0).t().tolist()))
    one_way = sum(1 for e in map(tuple, ei0.t().tolist()) if e not in rev and e[0] != e[1])
    assert one_way > ei0.size(1) // 2, "most edges have no reverse edge"
    ei, ew = _graphconv_weights(kind, ei0, n, seed)
    torch.manual_seed(seed)
    om = _randomise_biases(OConv(P.GraphConv(fin, h), act), seed)
    pm = _load(PConv(GraphConv(fin, h), act), om)
    consts = {"ei": ei} if ew is None else {"ei": ei, "ew": ew}
    if ew is None:
        drops = [{"ei": e} for (e,) in _drop_edges(ei, must=_hub_edges(ei))]
    else:
        drops = [{"ei": e, "ew": w} for e, w in _drop_edges(ei, (ew,), must=_hub_edges(ei))]
    _check(f"GraphConv directed {kind} {act}", om, pm, {"x": _x(n, fin, seed)}, consts, _x(n, h, seed + 1),
           gates=_gate, atol=2e-5, drops=drops)


@pytest.mark.parametrize("n,fin,h", [(40, 9, 16), (300, 16, 32), (150, 9, 10)])
def test_gat_conv_on_one_tensor(n, fin, h):
    """GATConv((F, F), H, add_self_loops=False) on ONE tensor (the homogeneous use ``HeteroConv`` makes of it):
    ``lin_src`` transforms both roles, ``lin_dst`` gets no gradient; a hub, nodes without
    in-edges; the input ``x`` receives gx_src + gx_dst."""
    from graph_hscn.nn import GATConv
    seed = {40: 43, 300: 301, 150: 150}[n]
    ei = multigraph(n, seed)
    assert int(torch.bincount(ei[1], minlength=n).min()) == 0 and int(torch.bincount(ei[1], minlength=n).max()) > 64
    torch.manual_seed(seed)
    om = _randomise_biases(OConv(P.GATConv((fin, fin), h)), seed)
    pm = _load(PConv(GATConv((fin, fin), h, add_self_loops=False)), om)
    drops = [{"ei": e} for (e,) in _drop_edges(ei, must=_hub_edges(ei))]
    _, (o32, g32, o64, g64, od, gd) = _check(f"GATConv one tensor n={n} F={fin} H={h}", om, pm, {"x": _x(n, fin, seed)},
                                              {"ei": ei}, _x(n, h, seed + 1), atol=2e-5, drops=drops)
    assert g64["p.op.lin_dst.weight"] is None and gd["p.op.lin_dst.weight"] is None


def test_global_mean_pool_backward():
    """Segments of 1, 7, 150 and 444 rows, an UNSORTED batch vector and an empty segment (id 2).  Teeth: one row moved
    out of the 7-, the 150- and the 444-row segment in turn (into the empty one): each must be rejected."""
    from graph_hscn.nn import global_mean_pool
    sizes = {0: 1, 1: 7, 3: 150, 4: 444}
    g = torch.Generator().manual_seed(3)
    batch = torch.cat([torch.full((c,), s) for s, c in sizes.items()])
    batch = batch[torch.randperm(batch.numel(), generator=g)]
    assert not bool((batch[1:] >= batch[:-1]).all())
    N, H, B = int(batch.numel()), 16, 5
    x = torch.randn(N, H, generator=g)
    gy = torch.randn(B, H, generator=g)

    def run(xx, bb, dtype):
        xx = xx.detach().clone().to(dtype).requires_grad_()
        y = P.global_mean_pool(xx, bb, B)
        y.backward(gy.to(dtype))
        return y.detach(), xx.grad

    y32, gx32 = run(x, batch, torch.float32)
    y64, gx64 = run(x, batch, torch.float64)
    xd = x.to(DEV).requires_grad_()
    yd = global_mean_pool(xd, batch.to(DEV), B)
    yd.backward(gy.to(DEV))
    print("[layered f64] global_mean_pool backward")
    assert close(yd, y32) and float(yd[2].abs().sum()) == 0.0
    assert referee(xd.grad, gx32, gx64, "global_mean_pool x") <= 1.0
    assert referee(yd, y32, y64, "global_mean_pool out") <= 1.0
    for seg in (1, 3, 4):
        row = int(torch.nonzero(batch == seg).flatten()[0])
        moved = batch.clone()
        moved[row] = 2
        yq, gq = run(x, moved, torch.float64)
        teeth({"x": xd.grad, "out": yd}, {"x": gx32, "out": y32}, {"x": gx64, "out": y64}, {"x": gq, "out": yq},
              f"global_mean_pool, a row out of segment {seg}")


class OHetero(nn.Module):
    """HeteroConv{(a,to,c): GAT bipartite, (c,to,c): GCN} -> the ``c`` rows (the oracle's stack-sum)."""

    def __init__(self, fin, h):
        super().__init__()
        self.op = P.HeteroConv({("a", "to", "c"): P.GATConv((fin, fin), h), ("c", "to", "c"): P.GCNConv(fin, h, add_self_loops=False)})

    def forward(self, xa, xc, ei_ac, ei_cc):
        return self.op({"a": xa, "c": xc}, {("a", "to", "c"): ei_ac, ("c", "to", "c"): ei_cc})["c"]


class PHetero(nn.Module):
    def __init__(self, fin, h):
        super().__init__()
        from graph_hscn.nn import GATConv, GCNConv, HeteroConv
        self.op = HeteroConv({("a", "to", "c"): GATConv((fin, fin), h, add_self_loops=False),
                              ("c", "to", "c"): GCNConv(fin, h, add_self_loops=False)})

    forward = OHetero.forward


def test_hetero_conv_two_relations_into_one_target():
    na, nc, fin, h, seed = 120, 23, 9, 16, 11
    g = torch.Generator().manual_seed(seed)
    ei_ac = torch.stack([torch.randint(0, na, (260,), generator=g), torch.randint(0, nc - 2, (260,), generator=g)])
    ei_cc = multigraph(nc, seed, hub=0)
    torch.manual_seed(seed)
    om = _randomise_biases(OHetero(fin, h), seed)
    pm = _load(PHetero(fin, h), om)
    x = {"xa": _x(na, fin, seed), "xc": _x(nc, fin, seed + 1)}
    drops = [{"ei_ac": e, "ei_cc": ei_cc} for (e,) in _drop_edges(ei_ac)]
    _, (o32, g32, o64, g64, od, gd) = _check("HeteroConv GAT(a->c) + GCN(c->c)", om, pm, x, {"ei_ac": ei_ac, "ei_cc": ei_cc},
                                              _x(nc, h, seed + 2), atol=2e-5, drops=drops)
    assert all(v is not None for v in gd.values()), "both relations' parameters and both sources receive gradients"
    drops = [{"ei_ac": ei_ac, "ei_cc": e} for (e,) in _drop_edges(ei_cc)]
    _check("HeteroConv GAT(a->c) + GCN(c->c), a c->c edge dropped", om, pm, x, {"ei_ac": ei_ac, "ei_cc": ei_cc},
           _x(nc, h, seed + 2), atol=2e-5, drops=drops)


# ---- needs_input_grad: frozen leaves switch kernels / workspaces off; what remains is the same kernels on the same data
def _run_frozen(make, x, consts, gy, freeze_x=(), freeze_p=()):
    pm = make()
    for n_, p in pm.named_parameters():
        if any(n_.endswith(f) for f in freeze_p):
            p.requires_grad_(False)
    xs = {k: v.to(DEV).requires_grad_(k not in freeze_x) for k, v in x.items()}
    out = pm(**xs, **_cast(consts, torch.float32, DEV))
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), grads_of(pm, **xs)


def _frozen_cases(kind):
    from graph_hscn.nn import BatchNorm1d, GATConv, GCNConv, GraphConv, LayerNorm
    from graph_hscn.nn import functional as Fh
    n, fin, h = 90, 9, 16
    ei = multigraph(n, 5, hub=0)
    x, gy = {"x": _x(n, fin, 5)}, _x(n, h, 6)

    def seeded(f):
        def make():
            torch.manual_seed(17)
            return _randomise_biases(f(), 17).to(DEV)
        return make

    if kind == "linear":
        return seeded(lambda: PLinear(fin, h, "tanh")), x, {}, gy, ("op.weight",), ("op.bias",)
    if kind == "gcn":
        return seeded(lambda: PConv(GCNConv(fin, h, add_self_loops=False), "elu")), x, {"ei": ei}, gy, ("lin.weight",), ("op.bias",)
    if kind == "graphconv":
        ew = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(1)) + 0.25
        return (seeded(lambda: PConv(GraphConv(fin, h), "tanh")), x, {"ei": ei, "ew": ew}, gy,
                ("lin_rel.weight", "lin_root.weight"), ("lin_rel.bias",))
    if kind == "gat":
        return (seeded(lambda: PConv(GATConv((fin, fin), h, add_self_loops=False))), x, {"ei": ei}, gy,
                ("lin_src.weight", "att_src", "att_dst"), ("op.bias",))
    if kind in ("gatloop_narrow", "gatloop_wide"):
        T = int(Fh.GAT_NARROW_MAX_DEGREE)
        ring = torch.arange(n)
        e2 = torch.stack([(ring + 1) % n, ring])                              # in-degree 1 <= T: the narrow-row kernels
        if kind == "gatloop_wide":                                           # one row above T: the wave-per-row kernels
            e2 = torch.cat([e2, torch.stack([10 + torch.arange(T + 1), torch.zeros(T + 1, dtype=torch.long)])], 1)
        return (seeded(lambda: PConv(GATConv(fin, h), "relu")), x, {"ei": e2}, gy,
                ("lin_src.weight", "att_src", "att_dst"), ("op.bias",))
    norm = LayerNorm if kind == "layernorm" else BatchNorm1d

    class PNorm(nn.Module):
        def __init__(self):
            super().__init__()
            self.op = norm(h)

        def forward(self, x):
            return self.op(x)

    def make():
        torch.manual_seed(17)
        m = PNorm()
        with torch.no_grad():
            m.op.weight.add_(torch.randn(h) * 0.3)
            m.op.bias.add_(torch.randn(h) * 0.3)
        return m.to(DEV)
    return make, {"x": _x(n, h, 5) * 3 + 1}, {}, gy, ("op.weight",), ("op.bias",)


@pytest.mark.parametrize("kind", ["linear", "gcn", "graphconv", "gat", "gatloop_narrow", "gatloop_wide", "layernorm",
                                  "batchnorm"])
def test_needs_input_grad_branches_leave_the_other_gradients_bit_identical(kind, monkeypatch):
    """(a) the input without grad, (b) the weights frozen, (c) the bias frozen -- and, where the module can be built
    without one and the gradients do not depend on it, absent: the gradients that remain are ``torch.equal`` to the
    all-gradients run, the frozen leaves' ``.grad`` is None."""
    make, x, consts, gy, weights, bias = _frozen_cases(kind)
    if kind.startswith("gatloop"):
        from graph_hscn.nn import functional as Fh
        names = []
        real = Fh.call
        monkeypatch.setattr(Fh, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    out_all, g_all = _run_frozen(make, x, consts, gy)
    if kind.startswith("gatloop"):
        assert ("hscn_gat_loop_fwd" in names) == (kind == "gatloop_narrow")
        assert ("hscn_gat_segment_fwd" in names) == (kind == "gatloop_wide")
    assert all(v is not None for k, v in g_all.items() if not k.endswith("lin_dst.weight")), g_all.keys()
    for tag, fx, fp in (("input", ("x",), ()), ("weights", (), weights), ("bias", (), bias),
                        ("input+weights", ("x",), weights)):
        out, g = _run_frozen(make, x, consts, gy, fx, fp)
        assert torch.equal(out, out_all), (kind, tag)
        for k, v in g_all.items():
            frozen = (k == "x.x" and fx) or any(k.endswith(f) for f in fp)
            if frozen or v is None:
                assert g[k] is None, (kind, tag, k)
            else:
                assert g[k] is not None and torch.equal(g[k], v), (kind, tag, k)


@pytest.mark.parametrize("kind", ["linear", "gcn", "gat"])
def test_module_without_bias_has_the_gradients_of_the_module_with_one(kind):
    """``bias=False`` with an identity epilogue: the output loses the bias, no gradient depends on it -- the gradients
    of x and of the weights are bit-identical to the module with a bias, through the kernels' bias-less variants."""
    from graph_hscn.nn import GATConv, GCNConv
    n, fin, h = 90, 9, 16
    ei = multigraph(n, 5, hub=0)
    x, gy = {"x": _x(n, fin, 5)}, _x(n, h, 6)
    build = {"linear": lambda b: PLinear(fin, h, "identity", bias=b),
             "gcn": lambda b: PConv(GCNConv(fin, h, add_self_loops=False, bias=b)),
             "gat": lambda b: PConv(GATConv((fin, fin), h, add_self_loops=False, bias=b))}[kind]
    consts = {} if kind == "linear" else {"ei": ei}

    def make(b):
        def f():
            torch.manual_seed(23)
            return _randomise_biases(build(b), 23).to(DEV)
        return f

    out_b, g_b = _run_frozen(make(True), x, consts, gy)
    out_n, g_n = _run_frozen(make(False), x, consts, gy)
    bias = g_b.pop("p.op.bias")
    assert bias is not None and "p.op.bias" not in g_n and set(g_n) == set(g_b)
    for k, v in g_b.items():
        assert (v is None and g_n[k] is None) or torch.equal(g_n[k], v), (kind, k)
    assert not torch.equal(out_b, out_n)


# --------------------------------------------------------------------------- #
# C. models on engine="layered"
# --------------------------------------------------------------------------- #
class _HB(dict):
    """The minimum of a batch ``HSCN._forward_layered`` reads."""

    def __init__(self, batch_local, num_graphs):
        super().__init__()
        self.num_graphs = num_graphs

        class L:
            batch = batch_local
        self["local"] = L()


class OHSCN(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, xl, xv, eis, batch_local, B):
        return self.m({"local": xl, "virtual": xv}, eis, batch_local, B)


class PHSCN(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, xl, xv, eis, batch_local, B):
        return self.m({"local": xl, "virtual": xv}, eis, _HB(batch_local, B))


def _hscn_gates(m):
    g = list(m.m.convs)                      # every HeteroConv's outputs (both node types) feed the hard ReLU
    return g + [m.m.lin_1]                   # and lin_1 the head's ReLU


def _hscn_pair(combo, F_, H, C, L, seed):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(seed)
    om = _randomise_biases(OHSCN(OM.HSCN(*combo, OM.ACT["relu"], F_, H, C, L)), seed, 0.1)
    pm = PHSCN(HSCN(*combo, ACT_DICT["relu"], F_, H, C, L))
    pm = _load(pm, om)
    pm.m.engine = "layered"
    return om, pm


def _hscn_check(what, combo, name, B, K, H, L, C, seed):
    from tests.helpers import hetero_batch
    b, _ = hetero_batch(name, B, K, seed)
    F_ = b["x_dict"]["local"].size(1)
    om, pm = _hscn_pair(combo, F_, H, C, L, seed)
    x = {"xl": b["x_dict"]["local"], "xv": b["x_dict"]["virtual"]}
    consts = {"eis": b["edge_index_dict"], "batch_local": b["batch_local"], "B": B}
    gy = torch.randn(B, C, generator=torch.Generator().manual_seed(seed + 1))
    drops = None
    if what in CANCELLING:                   # teeth of the derived bound: one local -> local edge removed
        eis = b["edge_index_dict"]
        ll = ("local", "to", "local")
        drops = [dict(consts, eis={**eis, ll: e}) for (e,) in _drop_edges(eis[ll])]
    worst, res = _check(what, om, pm, x, consts, gy, gates=_hscn_gates, atol=ATOL, rtol=RTOL, drops=drops,
                        chain_extra=int(b["batch_local"].numel()))          # the mean pool's segment: at most N rows
    assert pm.m.last_engine == "layered"
    return worst, res, (om, pm)


@pytest.mark.parametrize("H", [16, 32])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("ll,vv", [("GCN", "GCN"), ("GCN", "GAT"), ("GAT", "GCN"), ("GAT", "GAT")])
def test_hscn_relation_combinations(ll, vv, L, H):
    """lv = GAT with ll, vv in {GCN, GAT} on a PCQM-Contact-shaped batch of 4 graphs, K = 8: prediction at 1e-5, every
    parameter gradient through the referee with the oracle's None pattern -- under DESIGN.md section 2's semantics a
    homogeneous GAT relation's ``lin_dst`` has no gradient on either side."""
    seed = 100 + 10 * L + H
    _, (o32, g32, o64, g64, od, gd), _ = _hscn_check(f"HSCN GAT/{ll}/{vv} L={L} H={H}", ("GAT", ll, vv), "pcqm_contact",
                                                     4, 8, H, L, 3, seed)
    for k in gd:
        if k.endswith("lin_dst.weight") and ("local__to__local" in k or "virtual__to__virtual" in k):
            assert gd[k] is None and g64[k] is None, k
    if ll == "GAT":
        assert gd["p.m.convs.0.convs.local__to__local.lin_src.weight"] is not None


@pytest.mark.parametrize("ll,vv", [("GCN", "GCN"), ("GCN", "GAT"), ("GAT", "GCN"), ("GAT", "GAT")])
def test_hscn_engine_choice_for_the_relation_combinations(ll, vv):
    """On a real HeteroBatch that qualifies for the graph-resident engine (H = 16, F = 9): ``engine="auto"`` takes it
    for GAT/GCN/GCN only and the layered operators for the other three, for which ``engine="resident"`` and
    ``ResidentTrainStep`` raise."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.step import ResidentTrainStep
    K = 8
    graphs = make_dataset("pcqm_contact", 4, seed=2)
    rng = np.random.default_rng(2)
    hb = HeteroBatch.from_data_list([hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]).to(DEV)
    torch.manual_seed(0)
    pm = HSCN("GAT", ll, vv, ACT_DICT["relu"], 9, 16, 1, 2).to(DEV)
    default = (ll, vv) == ("GCN", "GCN")
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(hb.x_dict, hb.edge_index_dict, hb)
    assert out.shape == (4, 1)
    assert pm.last_engine == ("resident" if default else "layered")
    if default:
        return
    # the same batch and widths qualify with GAT/GCN/GCN (above), so the relations are what is refused: the message
    # names the combination the resident launches serve
    pm.engine = "resident"
    with pytest.raises(RuntimeError, match="GAT/GCN/GCN relations"):
        pm(hb.x_dict, hb.edge_index_dict, hb)
    pm.engine = "auto"
    with pytest.raises(RuntimeError, match="GAT/GCN/GCN relations"):
        ResidentTrainStep(pm, hb, "l1")


@pytest.mark.parametrize("name,H,L", [("pcqm_contact", 128, 2), ("pcqm_contact", 8, 2)])
def test_hscn_where_layered_is_the_only_engine(name, H, L):
    """The default GAT/GCN/GCN model outside the one-launch envelopes: H = 128, and F > H (F = 9, H = 8)."""
    _hscn_check(f"HSCN GAT/GCN/GCN H={H} (layered only)", ("GAT", "GCN", "GCN"), name, 4, 8, H, L, 3, 200 + H)


# ---- SCN: every layered MinCUT route
class OSCN(nn.Module):
    """The oracle's stage-A body per graph (gcn_norm(add_self_loops=True), forward, mc + o), losses meaned over the
    graphs -> [S of every node (flat), mean mc, mean o]."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, graphs):
        Ss, mc, o = [], 0.0, 0.0
        for x, ei in graphs:
            S, a, b_ = scn_step_in_dtype(self.m, x, ei)
            Ss.append(S.flatten())
            mc, o = mc + a, o + b_
        return torch.cat(Ss + [(mc / len(graphs)).view(1), (o / len(graphs)).view(1)])


class PSCN(nn.Module):
    def __init__(self, m, route):
        super().__init__()
        self.m, self.route = m, route

    def forward(self, graphs):
        from graph_hscn.data import Batch, Data
        from graph_hscn.nn import gcn_norm
        if self.route == "dense-ragged":
            big = Batch.from_data_list([Data(x=x.cpu(), edge_index=ei.cpu()) for x, ei in graphs]).to(DEV)
            S, mc, o = self.m.forward_graphs(big)
        else:
            big = Batch.from_data_list([Data(x=x.cpu(), edge_index=ei.cpu()) for x, ei in graphs]).to(DEV)
            ei, ew = gcn_norm(big.edge_index, None, big.num_nodes, add_self_loops=True)
            node_ptr = big.ptr.to(torch.int32) if self.route == "sparse-batched" else None
            S, mc, o, _ = self.m(big.x.float(), ei, ew, node_ptr=node_ptr)
        assert self.m.last_route == self.route.split("-batched")[0], self.m.last_route
        return torch.cat([S.flatten(), mc.view(1), o.view(1)])


def _scn_gates(act):
    def gates(m):
        if act != "relu":
            return []
        return [getattr(m.m.mp, f"module_{2 * i}") for i in range(m.m.mp._n)]
    return gates


def _scn_graphs(sizes, seed, directed):
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    rng = np.random.default_rng(seed)
    graphs = [make_graph(rng, SHAPES["pascalvoc_sp"], n=nn_) for nn_ in sizes]
    if directed:
        # every other graph loses one direction of a third of its edges: symmetric and directed graphs mixed
        for gi in range(0, len(graphs), 2):
            ei = graphs[gi].edge_index
            keep = torch.from_numpy(rng.random(ei.size(1)) > 0.33) | (ei[0] > ei[1])
            graphs[gi].edge_index = ei[:, keep].contiguous()
    return [(g.x.float(), g.edge_index) for g in graphs]


SCN_SEEDS = {(16, (40, 7, 129), 2): 33}      # where the default seed does not satisfy the kink guard


@pytest.mark.parametrize("units,act", [([16], "elu"), ([16, 16], "relu")])
@pytest.mark.parametrize("route,K,sizes,adj,directed", [
    ("sparse", 4, (57,), None, False),
    ("sparse", 16, (130,), None, True),
    ("sparse-batched", 16, (40, 7, 129), None, True),
    ("dense", 16, (65,), None, False),
    ("dense", 4, (130,), None, True),
    ("dense-ragged", 16, (40, 7, 129), "u8", True),
    ("dense-ragged", 16, (40, 7, 129), "f32", True),
    ("dense-ragged", 4, (64, 65, 2), "u8", False),
])
def test_scn_layered_routes(route, K, sizes, adj, directed, units, act, monkeypatch):
    """Stage A through the layered operators on every MinCUT route -- sparse (single graph; batched with ``node_ptr``),
    dense, dense-ragged with byte and float adjacency on a batch that mixes symmetric and directed graphs -- against the
    oracle's per-graph loop: assignments and both losses at 1e-5, every parameter gradient of mean(mc + o) through the
    referee."""
    from graph_hscn.model.hscn import SCN
    if adj is not None:
        monkeypatch.setenv("HSCN_DENSE_ADJ", adj)
    seed = SCN_SEEDS.get((K, sizes, len(units)), K + len(sizes) + len(units))
    graphs = _scn_graphs(sizes, seed, directed)
    F_ = graphs[0][0].size(1)
    torch.manual_seed(seed)
    om = OSCN(OM.SCN(units, act, F_, K))
    pm = PSCN(SCN(units, act, F_, K, mincut_route="sparse" if route.startswith("sparse") else "dense"), route)
    pm = _load(pm, om)
    N = sum(sizes)
    gy = torch.cat([torch.zeros(N * K), torch.ones(2)])              # d(mc + o): S itself carries no gradient
    what = f"SCN {route} K={K} sizes={sizes} adj={adj} directed={directed} mp_units={units} {act}"
    drops = None
    if what in CANCELLING:                   # teeth of the derived bound: one edge of the largest graph removed
        big = max(range(len(graphs)), key=lambda i: graphs[i][0].size(0))
        drops = [{"graphs": [(gx, e if i == big else gei) for i, (gx, gei) in enumerate(graphs)]}
                 for (e,) in _drop_edges(graphs[big][1])]
    _check(what, om, pm, {}, {"graphs": graphs}, gy, gates=_scn_gates(act), drops=drops,
           chain_extra=len(sizes) * (max(sizes) + K + 4))     # the MinCUT contractions: sums over a graph's nodes, clusters
    pm.m.check_adjacency()


# ---- MPNN
class OGatLoops(P.GATConv):
    """PyG GATConv(F, H) with its default self loops, restated as tests/test_gpu_gat_self_loops.py does: the bipartite
    oracle with ONE transform on ``with_self_loops(edge_index)``."""

    def __init__(self, fin, h):
        super().__init__((fin, fin), h)
        self.lin_dst = self.lin_src

    def forward(self, x, ei):
        from graph_hscn.structure import with_self_loops
        return super().forward((x, x), with_self_loops(ei, x.size(0)))


class OMPNN(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, ei, batch, B, masks=None):
        return self.m(x, ei, batch, B, masks=masks)


class PMPNN(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, ei, batch, B, masks=None):
        class _B:
            pass
        b = _B()
        b.x, b.edge_index, b.batch, b.num_graphs = x, ei, batch, B
        return self.m(b)


def _mpnn_pair(conv, act, F_, H, C, L, dropout, bn, ln, seed):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(seed)
    o = OM.MPNN(OM.ACT[act], F_, H, C, L, dropout, use_batch_norm=bn, use_layer_norm=ln)
    if conv == "gat":
        dims = [F_] + [H] * (L - 1) + [C]
        o.conv_layers = nn.ModuleList(OGatLoops(dims[i], dims[i + 1]) for i in range(L))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n_, p in o.named_parameters():
            if n_.endswith("bias") or "bns" in n_ or "lns" in n_:
                p.add_(torch.randn(p.shape, generator=g) * 0.2)
    om = OMPNN(o)
    p = MPNN(CONV_DICT[conv], ACT_DICT[act], F_, H, C, L, dropout, use_batch_norm=bn, use_layer_norm=ln)
    pm = _load(PMPNN(p), om)
    pm.m.engine = "layered"
    return om, pm


def _mpnn_gates(bn, ln, act):
    def gates(m):
        g = list(m.m.conv_layers[:-1])                                # F.relu(conv(x))
        if act == "relu" and ln:
            g += list(m.m.lns)                                        # the configured activation after the norm
        return g
    return gates


@pytest.mark.parametrize("conv", ["gcn", "gat"])
@pytest.mark.parametrize("mode", ["plain", "ln", "bn+ln", "dropout"])
def test_mpnn_layered(conv, mode):
    """The MPNN baseline on the layered operators, conv_type gcn and gat: plain; LayerNorm; BatchNorm + LayerNorm in
    training mode over TWO steps (the running statistics move, the second step's gradients are checked and the
    buffers compared); dropout p = 0.2 with the library's mask recovered on the device and fed to both oracles."""
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.nn import functional as Fh
    bn, ln = mode == "bn+ln", mode in ("ln", "bn+ln")
    p_drop = 0.2 if mode == "dropout" else 0.0
    act = {"plain": "relu", "ln": "relu", "bn+ln": "elu", "dropout": "tanh"}[mode]
    seed = 40
    B, F_, H, C, L = 4, 9, 16, 5, 3
    b = Batch.from_data_list(make_dataset("pcqm_contact", B, seed=seed))
    om, pm = _mpnn_pair(conv, act, F_, H, C, L, p_drop, bn, ln, seed)
    om.train(), pm.train()
    consts = {"ei": b.edge_index, "batch": b.batch, "B": B}
    if mode == "dropout":
        pm.m.dropout_seed = 1234
        ones = torch.ones(b.x.size(0), H, device=DEV)
        consts["masks"] = [(Fh.dropout(ones, p_drop, True, seed=1234 + i) != 0).float().cpu() for i in range(L - 1)]
    steps = 2 if bn else 1
    x = {"x": b.x.float()}
    gy = torch.randn(B, C, generator=torch.Generator().manual_seed(seed + 1))
    what = f"MPNN {conv} {mode}"
    tol = dict(atol=2e-5, rtol=1e-4) if (bn or ln) else dict(atol=ATOL, rtol=RTOL)      # test_gpu_mpnn.py's forward bars
    drops = None
    if what in CANCELLING:                   # teeth of the derived bound: one edge of the batch removed
        drops = [dict(consts, ei=e) for (e,) in _drop_edges(b.edge_index)]
    _check(what, om, pm, x, consts, gy, gates=_mpnn_gates(bn, ln, act), drops=drops, steps=steps,
           chain_extra=int(b.x.size(0)), **tol)                 # chain_extra: the mean pool's segment, at most N rows
    assert pm.m.last_engine == "layered"
    if bn:                                   # the running statistics after the two steps, against the float32 oracle's
        o = copy.deepcopy(om)
        for _ in range(steps):
            o(b.x.float(), **consts).backward(gy)
        pbuf = dict(pm.named_buffers())
        for n_, bo in o.named_buffers():
            assert close(pbuf[n_].float(), bo.float(), atol=1e-5, rtol=1e-5), n_
