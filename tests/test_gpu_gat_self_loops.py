"""GATConv(in, out) with PyG's default self-loop handling on the HIP path (csrc/gat_loops.hip: hscn_gat_loop_fwd /
_bwd_dst / _bwd_src; above nn.functional.GAT_NARROW_MAX_DEGREE the wave-per-row kernels of csrc/gat.hip over the
explicit-loop relation) and the MPNN baseline built from it (CONV_DICT["gat"]).

Reference: ``oracle.pyg_ops.GATConv((F, F), H)`` as it stands -- the bipartite operator without loops -- with ONE weight
in both transforms, ``x_src = x_dst = x`` and the edge list ``structure.with_self_loops(edge_index, N)`` computed on the
CPU (tests/test_gat_self_loops_host.py shows that this is the operator), in float32 for the forward at north_star's
1e-5 and after ``.double()`` for the gradients under ``helpers.f64_close`` / ``check_f64``, with the way of counting
``n`` of tests/test_gpu_ops_f64.py::test_gat_backward."""
import copy

import pytest
import torch
import torch.nn as nn

from oracle import models as OM
from oracle import pyg_ops as P
from tests.helpers import DEV, check_f64, close, f64_close

pytestmark = pytest.mark.gpu

F_IN = 9
N_NODES = 301          # odd: not a multiple of the 4, 8 or 16 rows a wave covers
WIDTHS = [16, 32, 10, 3, 64]


def _threshold():
    from graph_hscn.nn import functional as Fh
    return int(Fh.GAT_NARROW_MAX_DEGREE)


def _cpu_loops(ei, n):
    from graph_hscn.structure import with_self_loops
    return with_self_loops(ei.cpu(), n)


def _graph(n, maxdeg):
    """A ring over nodes [0, n-20) (in-degree 2) with: three input loops on node 3 (raw in-degree 5, the largest of
    the base graph), the edge 0 -> 1 three times, nodes n-20.. isolated except n-5, whose only input edge is a loop,
    and node 10 raised to a raw in-degree of exactly ``maxdeg`` (None: left alone) by edges from distinct sources."""
    m = n - 20
    i = torch.arange(m)
    ei = torch.cat([torch.stack([(i + 1) % m, i]), torch.stack([(i - 1) % m, i]),
                    torch.tensor([[3, 3, 3, 0, 0, n - 5], [3, 3, 3, 1, 1, n - 5]])], 1)
    if maxdeg is not None:
        assert 5 < maxdeg < m - 20
        extra = maxdeg - 2
        srcs = 20 + torch.arange(extra)                       # distinct, none of them 9, 10 or 11
        ei = torch.cat([ei, torch.stack([srcs, torch.full((extra,), 10)])], 1)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(n))
    return ei[:, perm].contiguous()                           # edge order is not sorted by anything


def _case_degree(case):
    T = _threshold()
    return {"small": None, "below": T - 1, "at": T, "above": T + 1, "hub3x": 3 * T}[case]


def _oracle(F, H, seed):
    torch.manual_seed(seed)
    o = P.GATConv((F, F), H)
    o.lin_dst = o.lin_src                  # one transform, as PyG builds GATConv(int, out)
    with torch.no_grad():
        o.bias.normal_()
    return o


def _product(o, F, H):
    from graph_hscn.nn.conv import GATConv
    pc = GATConv(F, H).to(DEV)
    pc.load_state_dict(o.state_dict())
    return pc


class _Spy:
    """Names of the C-ABI entries issued through nn.functional while active."""

    def __init__(self, monkeypatch):
        from graph_hscn.nn import functional as Fh
        self.names = []
        real = Fh.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(Fh, "call", call)


def _act64(t, act):
    if act == "relu":
        return t.clamp_min(0)
    if act == "elu":
        return torch.where(t > 0, t, torch.expm1(t))
    return t


@pytest.mark.parametrize("case", ["small", "below", "at", "above", "hub3x"])
@pytest.mark.parametrize("H", WIDTHS)
def test_forward_matches_the_float32_oracle(H, case, monkeypatch):
    from graph_hscn.structure import Relation
    n = N_NODES
    maxdeg = _case_degree(case)
    ei = _graph(n, maxdeg)
    o = _oracle(F_IN, H, 10 + H)
    x = torch.randn(n, F_IN, generator=torch.Generator().manual_seed(H))
    yo = torch.relu(o((x, x), _cpu_loops(ei, n))).detach()
    pc = _product(o, F_IN, H)
    spy = _Spy(monkeypatch)
    eid = ei.to(DEV)
    with torch.no_grad():
        yd = pc(x.to(DEV), eid, act="relu")
        yr = pc(x.to(DEV), Relation(eid, n, n), act="relu")          # a prebuilt Relation of the raw list
    rel = Relation(eid, n, n)
    assert rel.max_in_degree == (5 if maxdeg is None else maxdeg)
    narrow = case in ("small", "below", "at")
    assert ("hscn_gat_loop_fwd" in spy.names) == narrow and ("hscn_gat_segment_fwd" in spy.names) == (not narrow)
    d = (yd.cpu() - yo).abs()
    print(f"gat loops fwd H={H} {case}: max abs diff {float(d.max()):.3e}, max |ref| {float(yo.abs().max()):.3f}")
    assert close(yd, yo)
    assert torch.equal(yr, yd)


@pytest.mark.parametrize("H", WIDTHS)
def test_forward_without_edges(H):
    """E = 0: every node sees only its loop, alpha = 1 / (1 + 1e-16), out = h + bias."""
    n = 37
    ei = torch.zeros(2, 0, dtype=torch.int64)
    o = _oracle(F_IN, H, 20 + H)
    x = torch.randn(n, F_IN, generator=torch.Generator().manual_seed(H))
    xo = x.clone().requires_grad_()
    yo = o((xo, xo), _cpu_loops(ei, n))
    pc = _product(o, F_IN, H)
    xd = x.to(DEV).requires_grad_()
    yd = pc(xd, ei.to(DEV))
    assert close(yd, yo)
    assert close(yo, (x @ o.lin_src.weight.t() + o.bias).detach())
    gy = torch.randn(n, H, generator=torch.Generator().manual_seed(1))
    yo.backward(gy)
    yd.backward(gy.to(DEV))
    # alpha is constant: the gradient is that of a linear layer (float32 oracle, operator-level bar of test_gpu_ops.py)
    assert close(xd.grad, xo.grad, atol=1e-5, rtol=1e-4)
    assert close(pc.lin_src.weight.grad, o.lin_src.weight.grad, atol=1e-4, rtol=1e-4)
    assert close(pc.bias.grad, o.bias.grad, atol=1e-4, rtol=1e-4)


LEAVES = ["x", "W", "att_src", "att_dst", "bias"]


def _grads64(o, x, ei_used, gy, act):
    """Float64 gradients of every leaf through the oracle over ``ei_used`` (loops are the caller's business)."""
    o64 = copy.deepcopy(o).double()
    assert o64.lin_dst is o64.lin_src
    x64 = x.double().requires_grad_()
    _act64(o64((x64, x64), ei_used), act).backward(gy.double())
    return {"x": x64.grad, "W": o64.lin_src.weight.grad, "att_src": o64.att_src.grad.view(-1),
            "att_dst": o64.att_dst.grad.view(-1), "bias": o64.bias.grad}


def _n_of(name, n_base, N):
    # tests/test_gpu_ops_f64.py::test_gat_backward: the parameter gradients add a sum over the rows
    return n_base + (N if name in ("W", "att_src", "att_dst") else 0)


def _scale_mag(ref):
    return torch.full_like(ref, float(ref.abs().max()))


@pytest.mark.parametrize("side", ["narrow", "wide"])
@pytest.mark.parametrize("H,act", [(16, "elu"), (32, "identity"), (10, "elu"), (3, "identity"), (64, "identity")])
def test_backward_of_every_leaf_against_float64(H, act, side, monkeypatch):
    """Both sides of the dispatch (largest raw in-degree exactly at the threshold / one above it).  Teeth, in float64 on
    the CPU before the GPU is touched: the gradients with the appended loop left out, and with the input loops kept,
    must each lie outside the bound for every leaf the graph reaches (x, W, att_src, att_dst; with act = identity the
    bias gradient is sum(gy) whatever the graph, so it has no teeth and gets ``f64_close`` alone)."""
    n, I, slope = N_NODES, F_IN, 0.2
    T = _threshold()
    maxdeg = T if side == "narrow" else T + 1
    ei = _graph(n, maxdeg)
    assert int((ei[0] == ei[1]).sum()) == 4
    ei_ok = _cpu_loops(ei, n)
    ei_no_loop = ei[:, ei[0] != ei[1]]
    ei_kept = torch.cat([ei, torch.arange(n).expand(2, -1)], 1)
    teeth_leaves = ["x", "W", "att_src", "att_dst"]
    used = None
    for seed in range(1000 + H, 1000 + H + 8):
        o = _oracle(I, H, seed)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, I, generator=g)
        gy = torch.randn(n, H, generator=g)
        ref = _grads64(o, x, ei_ok, gy, act)
        wrong = {"loop left out": _grads64(o, x, ei_no_loop, gy, act),
                 "input loops kept": _grads64(o, x, ei_kept, gy, act)}
        with torch.no_grad():
            h = x.double() @ o.lin_src.weight.double().t()
            a_s, a_d = h @ o.att_src.double().view(-1), h @ o.att_dst.double().view(-1)
            zmax = float((a_s[ei_ok[0]] + a_d[ei_ok[1]]).abs().max())
        n_base = (maxdeg + 1) + I + 2 * H + 16 + 2 * zmax
        seen = all(not f64_close(w[k], ref[k], _scale_mag(ref[k]), _n_of(k, n_base, n))
                   for w in wrong.values() for k in teeth_leaves)
        if seen:
            used = seed
            break
    assert used is not None, "no seed in eight gave wrong variants outside the bound"
    print(f"gat loops bwd H={H} {act} {side}: inputs drawn from seed {used}, n = {n_base:.1f}")

    pc = _product(o, I, H)
    spy = _Spy(monkeypatch)
    xd = x.to(DEV).requires_grad_()
    yd = pc(xd, ei.to(DEV), act=act)
    yd.backward(gy.to(DEV))
    want = ("hscn_gat_loop_bwd_dst", "hscn_gat_loop_bwd_src") if side == "narrow" else \
        ("hscn_gat_segment_bwd_dst", "hscn_gat_segment_bwd_src")
    assert all(w in spy.names for w in want), spy.names
    got = {"x": xd.grad, "W": pc.lin_src.weight.grad, "att_src": pc.att_src.grad.view(-1),
           "att_dst": pc.att_dst.grad.view(-1), "bias": pc.bias.grad}
    for k in LEAVES:
        r = ref[k]
        d = float((got[k].cpu().double() - r).abs().max())
        lim = 3 * _n_of(k, n_base, n) * 2.0 ** -24 * float(r.abs().max())
        print(f"  {k}: max abs diff {d:.3e}, limit {lim:.3e}")
    for k in LEAVES:
        r = ref[k]
        what = f"gat loops bwd {H} {act} {side} {k}"
        if k in teeth_leaves:
            for w in wrong.values():
                check_f64(got[k], r, _scale_mag(r), _n_of(k, n_base, n), w[k], what=what)
        else:
            assert f64_close(got[k], r, _scale_mag(r), _n_of(k, n_base, n), what=what)


@pytest.mark.parametrize("H", [16, 10])
def test_launches_replay_from_a_captured_graph(H):
    """Forward and backward of the narrow-row path recorded with torch.cuda.graph replay bit-identically to the eager
    call: every shape is host-known (no boolean-mask indexing between the edge list and the launches)."""
    from graph_hscn.structure import Relation
    n = N_NODES
    ei = _graph(n, _threshold()).to(DEV)
    o = _oracle(F_IN, H, 30 + H)
    pc = _product(o, F_IN, H)
    g = torch.Generator().manual_seed(H)
    x = torch.randn(n, F_IN, generator=g).to(DEV).requires_grad_()
    gy = torch.randn(n, H, generator=g).to(DEV)
    rel = Relation(ei, n, n, both=True)
    assert rel.max_in_degree == _threshold()       # read (one synchronising copy) before the capture
    leaves = [x, pc.lin_src.weight, pc.att_src, pc.att_dst, pc.bias]

    def run():
        y = pc(x, rel, act="relu")
        return [y] + list(torch.autograd.grad(y, leaves, gy))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(["out", "g_x", "g_W", "g_att_src", "g_att_dst", "g_bias"], outs, eager):
            assert torch.equal(a, b), name


# --------------------------------------------------------------------------- #
# the MPNN baseline with conv_type "gat"
# --------------------------------------------------------------------------- #
class _RefMPNN(nn.Module):
    """model/mpnn.py:13-62 with conv = GATConv, composed from the oracle's GATConv (one weight in both transforms, edge
    list with loops) and the oracle's mean pool; the parameter names are the product's."""

    def __init__(self, F, H, C, L):
        super().__init__()
        dims = [(F, H)] + [(H, H)] * (L - 2) + [(H, C)]
        self.conv_layers = nn.ModuleList()
        for i, o_ in dims:
            c = P.GATConv((i, i), o_)
            c.lin_dst = c.lin_src
            self.conv_layers.append(c)
        self.zmax = 0.0
        self.kept = []

    def forward(self, x, ei_loops, batch, num_graphs):
        self.zmax = 0.0
        self.kept = []                    # per layer: (h, a_src, a_dst, the convolution's output with its gradient kept)
        for k, c in enumerate(self.conv_layers):
            with torch.no_grad():
                h = c.lin_src(x)
                a_s, a_d = (h * c.att_src.view(-1)).sum(-1), (h * c.att_dst.view(-1)).sum(-1)
                self.zmax = max(self.zmax, float(a_s.abs().max() + a_d.abs().max()))
            x = c((x, x), ei_loops)
            if x.requires_grad:
                x.retain_grad()
            self.kept.append((h, a_s, a_d, x))
            if k + 1 < len(self.conv_layers):
                x = torch.relu(x)
        return P.global_mean_pool(x, batch, num_graphs)

    def attention_grad_abs_sums(self, ei_loops, slope=0.2):
        """After a backward: per layer, (sum_e |gp_e| |h[src_e]|, sum_e |gp_e| |h[dst_e]|) with gp_e = dL/d(a_src[src_e] +
        a_dst[dst_e]) -- the gradients of att_src / att_dst evaluated on absolute values, f64_close's ``mag`` for a sum
        whose terms cancel (within a row sum_e alpha_e (d_e - sum alpha d) = 0: where every score of a row has one
        sign the leaky ReLU does not break the tie and dL/datt_dst is zero up to rounding)."""
        src, dst = ei_loops[0], ei_loops[1]
        out = []
        with torch.no_grad():
            for h, a_s, a_d, y in self.kept:
                pre = a_s[src] + a_d[dst]
                z = torch.where(pre > 0, pre, pre * slope)
                alpha = P.segment_softmax(z, dst, h.shape[0])
                d = (y.grad[dst] * h[src]).sum(-1)
                ts = torch.zeros(h.shape[0], dtype=h.dtype).index_add(0, dst, alpha * d)
                gp = (alpha * (d - ts[dst]) * torch.where(pre > 0, 1.0, slope)).abs()
                out.append((torch.zeros_like(h).index_add(0, src, gp.view(-1, 1) * h[src].abs()).sum(0),
                            torch.zeros_like(h).index_add(0, dst, gp.view(-1, 1) * h[dst].abs()).sum(0)))
        return out


def _peptides(B, seed):
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("peptides_func", B, seed=seed)
    return graphs, Batch.from_data_list(graphs)


def _dev(b):
    d = b.to(DEV)
    d.x = d.x.float()
    return d


def _mpnn_pair(seed, dropout=0.0):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(seed)
    om = _RefMPNN(9, 16, 10, 3)
    with torch.no_grad():
        for c in om.conv_layers:
            c.bias.normal_(0, 0.1)
    pm = MPNN(CONV_DICT["gat"], ACT_DICT["relu"], 9, 16, 10, 3, dropout).to(DEV)
    assert sorted(pm.state_dict()) == sorted(om.state_dict())
    pm.load_state_dict(om.state_dict())
    return om, pm


def test_mpnn_gat_evaluated_and_one_training_iteration():
    """MPNN(GATConv, relu, 9, 16, 10, 3) on a Peptides-shaped batch of 32: prediction and first-iteration loss at 1e-5
    against the float32 reference model, every parameter gradient against the float64 one.

    n of the gradient bound: the chain is L = 3 convolutions deep, each contributing test_gat_backward's count
    (deg + 1 entries, the transform's width, 2 H for the two dots, 16 for the softmax / epilogue roundings, 2 max|z|),
    plus the sum over the N rows behind every parameter gradient and the mean over the graph's nodes (<= N).
    mag: the float64 gradient's normwise scale as in test_gat_backward; for att_src / att_dst not below the same sum
    evaluated on absolute values (_RefMPNN.attention_grad_abs_sums) -- on this batch the hidden layer's dL/datt_dst is
    zero up to rounding (2.8e-16 in float64), and a bound scaled by a rounding residue bounds nothing.  A leaf keeps the
    teeth of check_f64 (the loop-less model's gradient must be rejected) where float64 can tell the two apart."""
    from graph_hscn.loss import criterion
    from graph_hscn.structure import Relation
    B = 32
    _, b = _peptides(B, seed=41)
    N = int(b.x.shape[0])
    ei_loops = _cpu_loops(b.edge_index, N)
    om, pm = _mpnn_pair(3)
    x32 = b.x.float()
    y = b.y.float()
    o64, bad = copy.deepcopy(om).double(), copy.deepcopy(om).double()
    # float32 reference
    pred_o = om(x32, ei_loops, b.batch, B)
    loss_o, _ = OM.criterion("cross_entropy", pred_o, y)
    # float64 reference and its loop-less twin (teeth of check_f64)
    l64, _ = OM.criterion("cross_entropy", o64(x32.double(), ei_loops, b.batch, B), y.double())
    l64.backward()
    zmax = o64.zmax
    lb, _ = OM.criterion("cross_entropy", bad(x32.double(), b.edge_index[:, b.edge_index[0] != b.edge_index[1]],
                                              b.batch, B), y.double())
    lb.backward()
    ref = {k: p.grad for k, p in o64.named_parameters()}
    dropped = {k: p.grad for k, p in bad.named_parameters()}
    mags = {k: _scale_mag(r) for k, r in ref.items()}
    for l, (m_s, m_d) in enumerate(o64.attention_grad_abs_sums(ei_loops)):
        for k, m_ in ((f"conv_layers.{l}.att_src", m_s), (f"conv_layers.{l}.att_dst", m_d)):
            mags[k] = torch.maximum(mags[k], m_.view_as(mags[k]))

    bd = _dev(b)
    maxdeg = Relation(bd.edge_index, N, N).max_in_degree
    assert maxdeg <= _threshold()                      # a molecule batch takes the narrow-row kernels
    pm.eval()
    with torch.no_grad():
        pred_e = pm(bd)
    assert pm.last_engine == "layered"
    print("mpnn gat eval: max abs diff", float((pred_e.cpu() - pred_o.detach()).abs().max()))
    assert close(pred_e, pred_o)
    pm.train()
    pred_d = pm(bd)
    loss_d, _ = criterion("cross_entropy", pred_d, bd.y)
    loss_d.backward()
    torch.cuda.synchronize()
    assert close(pred_d, pred_o)
    print("mpnn gat loss", float(loss_d.detach()), "oracle", float(loss_o.detach()))
    assert abs(float(loss_d.detach()) - float(loss_o.detach())) < 1e-5
    L = 3
    n = L * ((maxdeg + 1) + 16 + 2 * 16 + 16 + 2 * zmax) + 2 * N
    # (dL/datt_dst is zero or nearly so in every layer here -- the scores of a row share a sign -- with or without the
    # loops; its teeth are the operator test's, test_backward_of_every_leaf_against_float64)
    teeth = {k: not f64_close(dropped[k], ref[k], mags[k], n) for k in ref}
    assert all(t for k, t in teeth.items() if not k.endswith("att_dst")), teeth
    prod = dict(pm.named_parameters())
    assert sorted(prod) == sorted(ref)
    for k, r in ref.items():
        d = float((prod[k].grad.cpu().double() - r).abs().max())
        print(f"  {k}: max abs diff {d:.3e}, max |ref| {float(r.abs().max()):.3e}, "
              f"smallest limit {3 * n * 2.0 ** -24 * float(mags[k].min()):.3e}, teeth {teeth[k]}")
    for k, r in ref.items():
        if teeth[k]:
            check_f64(prod[k].grad, r, mags[k], n, dropped[k], what=k)
        else:
            assert f64_close(prod[k].grad, r, mags[k], n, what=k)


def test_mpnn_gat_trains_with_adam_and_dropout_is_deterministic():
    from graph_hscn.data import DataLoader
    from graph_hscn.train import train as T
    graphs, _ = _peptides(96, seed=43)
    _, pm = _mpnn_pair(5)
    before = {k: p.detach().clone() for k, p in pm.named_parameters()}
    opt = torch.optim.Adam(pm.parameters(), lr=1e-2)
    loader = DataLoader(graphs, batch_size=32)
    assert len(loader) == 3
    loss, _ = T.train_epoch(0, None, loader, pm, opt, "cross_entropy", None, 1, False)
    assert loss == loss and abs(loss) != float("inf")
    for k, p in pm.named_parameters():
        assert torch.isfinite(p).all(), k
        assert not torch.equal(p.detach(), before[k]), f"{k} did not move"
    # dropout with a pinned seed: the same mask on every call
    _, b = _peptides(32, seed=44)
    bd = _dev(b)
    _, pd = _mpnn_pair(6, dropout=0.2)
    pd.train()
    pd.dropout_seed = 1234
    with torch.no_grad():
        a1, a2 = pd(bd), pd(bd)
        pd.eval()
        e = pd(bd)
    assert torch.isfinite(a1).all() and torch.equal(a1, a2)
    assert not torch.equal(a1, e)


def test_resident_engines_refuse_the_gat_model_with_the_reason():
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.train.train_resident import fit_resident
    graphs, b = _peptides(12, seed=45)
    bd = _dev(b)
    _, pm = _mpnn_pair(7)
    pm.eval()
    with torch.no_grad():
        ref = pm(bd)
        pm.engine = "auto"
        out = pm(bd)
        assert pm.last_engine == "layered" and torch.equal(out, ref)
        pm.engine = "resident"
        with pytest.raises(RuntimeError, match="GATConv"):
            pm(bd)
    pm.engine = "layered"
    for g_ in graphs:
        g_.x = g_.x.float()
    tc = TrainingConfig("mpnn", "cross_entropy", "ap", epochs=1, eval_period=1, patience=50)
    cfg = OptimConfig("adamW", lr=0.01)
    assert not torch.cuda.is_current_stream_capturing()
    with pytest.raises(RuntimeError, match="GATConv"):
        fit_resident(None, cfg, tc, graphs[:8], [DataLoader(graphs[8:], batch_size=4)] * 2, pm, batch_size=4)
    assert not torch.cuda.is_current_stream_capturing()
