"""Global attention on the HIP path (csrc/attention.hip, nn/attention.py, nn/gps.py, model/gps.py) against the
plain-torch restatement of tests/attention_oracle.py.

Tolerances are the project's own (tests/helpers.py), no new constants:
  * the forward by ``check_f64``: |out - out64| <= 3 n_i 2^-24 mag_id with mag_id = sum_j p_ij |v_jd| and
    n_i = n_g + 4 + 2 (dh + 2) max_j a_ij, a_ij = scale sum_d |q_id| |k_jd|.  A score is a dot product of length dh:
    absolute error <= (dh + 2) u a_ij; it enters p_ij as a relative error twice (the score and the row maximum),
    beside the helper's softmax rule deg + 4 + |z| + |m| with |z|, |m| <= a.  The same bound must REJECT out64 with
    the single largest message p_ij v_j removed, out64 computed with the graph boundary off by one, and out64 computed
    with the heads taken from interleaved columns;
  * lse by ``f64_close``: the score error (dh + 2) u a, the sum of n_g exponentials (n_g + 4) u, the roundings of
    m + log l: n = n_g + dh + 6, mag = a + 1 + |lse64|;
  * every gradient, the module and the models by ``referee_all`` (float32 and float64 restatements on the CPU as the two
    oracles) with ``teeth``.

Shapes: with T = hscn_attention_tile() and C = hscn_attention_chunk(), one batch holds graphs of
n in {1, 2, T-1, T, T+1, C-1, C, C+1, 2C+1} nodes and one empty graph in the middle."""
import copy

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import MultiheadSelfAttention
from graph_hscn.nn.gps import GPSLayer
from tests import attention_oracle as AO
from tests import gps_oracle as GPSO
from tests.helpers import (DEV, KinkGuard, TermMagnitudes, check_f64, f64_close, grads_of, most_changed, referee_all,
                           teeth)

pytestmark = pytest.mark.gpu

HEAD_SHAPES = [(1, 4), (3, 8), (4, 24), (2, 64)]


def _sizes():
    T, C = int(_hip.lib().hscn_attention_tile()), int(_hip.lib().hscn_attention_chunk())
    return [1, 2, T - 1, T, T + 1, 0, C - 1, C, C + 1, 2 * C + 1]


def _ptr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)


def _hip_attention(qkv, ptr, heads, max_nodes=None, requires_grad=False):
    """(out, leaf) of the operator on the device."""
    q = qkv.to(DEV).requires_grad_(requires_grad)
    ptr32 = ptr.to(torch.int32).to(DEV)
    sizes = (ptr[1:] - ptr[:-1])
    mn = int(sizes.max()) if max_nodes is None else max_nodes
    return Fh.SelfAttentionFn.apply(q, ptr32, mn, heads), q


class _Spy:
    """Names of the C-ABI entries issued through nn.functional while active (tests/test_gpu_gat_self_loops.py's)."""

    def __init__(self, monkeypatch):
        self.names = []
        real = Fh.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(Fh, "call", call)


def _lse_of(qkv, ptr, heads):
    """The kernel's lse through the raw entry point (the autograd function keeps it to itself)."""
    q = qkv.to(DEV).contiguous()
    N, D = q.size(0), q.size(1) // 3
    ptr32 = ptr.to(torch.int32).to(DEV)
    out = torch.empty(N, D, device=DEV)
    lse = torch.empty(N, heads, device=DEV)
    _hip.call("hscn_attention_fwd", _hip.ptr(q), _hip.ptr(ptr32), N, ptr32.numel() - 1,
              int((ptr[1:] - ptr[:-1]).max()), heads, D // heads, _hip.ptr(out), _hip.ptr(lse),
              _hip.ptr(Fh.attention_flags(DEV)), _hip.stream())
    return out, lse


_CASES = {}


def _case(heads, dh):
    """Inputs and the float64 reference of one head shape, computed once and shared (never modified)."""
    key = (heads, dh)
    if key not in _CASES:
        sizes = _sizes()
        ptr = _ptr(sizes)
        g = torch.Generator().manual_seed(100 * heads + dh)
        N, D = int(ptr[-1]), heads * dh
        qkv = torch.randn(N, 3 * D, generator=g)
        g_out = torch.randn(N, D, generator=g)
        out64, lse64 = AO.forward(qkv.double(), ptr, heads)
        a, mag, n = AO.magnitudes(qkv, ptr, heads)
        _CASES[key] = dict(sizes=sizes, ptr=ptr, qkv=qkv, g_out=g_out, out64=out64, lse64=lse64, a=a, mag=mag, n=n,
                           n_out=n + 4 + 2 * (dh + 2) * a.repeat_interleave(dh, 1))
    return _CASES[key]


def _flag():
    return int(Fh.attention_flags(DEV).item())


# --------------------------------------------------------------------------- #
# 1. + 2. forward against float64, with the three kinds of teeth
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_forward_matches_float64_and_the_bound_has_teeth(heads, dh):
    c = _case(heads, dh)
    qkv, ptr, D = c["qkv"], c["ptr"], heads * dh
    what = f"attention forward heads={heads} dh={dh}"
    out, _ = _hip_attention(qkv, ptr, heads)
    assert out.shape == (qkv.size(0), D)
    where = AO.largest_message(qkv, ptr, heads)
    dropped = AO.drop_message(c["out64"], qkv, ptr, heads, where)
    check_f64(out, c["out64"], c["mag"], c["n_out"], dropped, what=what)
    # the graph boundary off by one: the first key of the next graph let in
    off = AO.forward(qkv.double(), ptr, heads, boundary=1)[0]
    assert not f64_close(out, off, c["mag"], c["n_out"]), f"{what}: the bound cannot see a boundary off by one"
    # heads from interleaved columns instead of contiguous ones (one head: the two layouts are the same layout)
    if heads > 1:
        inter = AO.forward(qkv.double(), ptr, heads, interleaved=True)[0]
        assert not f64_close(out, inter, c["mag"], c["n_out"]), f"{what}: the bound cannot tell the head layout"
    # lse, and the raw entry point gives the same bits as the autograd function
    out_raw, lse = _lse_of(qkv, ptr, heads)
    assert torch.equal(out_raw, out)
    assert f64_close(lse, c["lse64"], c["a"] + 1.0 + c["lse64"].abs(), c["n"] + dh + 6, what=what + " lse")
    # a graph of one node: out = v and lse = s_00, exactly
    assert c["sizes"][0] == 1
    assert torch.equal(out[0].cpu(), qkv[0, 2 * D:])
    s00 = (qkv[0, :D].double().view(heads, dh) * qkv[0, D:2 * D].double().view(heads, dh)).sum(1) * dh ** -0.5
    assert torch.allclose(lse[0].cpu().double(), s00, rtol=0, atol=3 * (dh + 2) * 2.0 ** -24 * float(c["a"][0].max()))
    assert _flag() == 0


def test_float32_torch_stays_far_inside_the_bound():
    """The bound is not vacuous the other way: torch's own float32 evaluation uses a small part of it."""
    c = _case(4, 24)
    out32 = AO.forward(c["qkv"], c["ptr"], 4)[0]
    lim = 3 * c["n_out"] * 2.0 ** -24 * c["mag"] + 1e-30
    assert float(((out32.double() - c["out64"]).abs() / lim).max()) < 0.5


# --------------------------------------------------------------------------- #
# 3. placement independence, bit for bit
# --------------------------------------------------------------------------- #
def _fwd_bwd(qkv, g_out, ptr, heads):
    out, leaf = _hip_attention(qkv, ptr, heads, requires_grad=True)
    out.backward(g_out.to(DEV))
    _, lse = _lse_of(qkv, ptr, heads)
    return out.detach(), lse, leaf.grad


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_a_graph_has_the_same_bits_wherever_it_stands(heads, dh):
    c = _case(heads, dh)
    qkv, g_out, sizes = c["qkv"], c["g_out"], [s for s in c["sizes"] if s]
    assert len(sizes) == 9
    ptr = _ptr(sizes)                                       # a batch of nine; the graph under test is the last
    n = sizes[-1]
    s = int(ptr[-2])
    full = _fwd_bwd(qkv, g_out, ptr, heads)
    again = _fwd_bwd(qkv, g_out, ptr, heads)                # two runs of the same launch
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    alone = _fwd_bwd(qkv[s:], g_out[s:], _ptr([n]), heads)
    other = qkv.clone()
    other[:s] = torch.randn(s, qkv.size(1), generator=torch.Generator().manual_seed(5))
    changed = _fwd_bwd(other, g_out, ptr, heads)
    for name, f, a, ch in zip(("out", "lse", "g_qkv"), full, alone, changed):
        assert torch.equal(f[s:], a), name
        assert torch.equal(f[s:], ch[s:]), name
        assert not torch.equal(f[:s], ch[:s]), name
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# 4. backward
# --------------------------------------------------------------------------- #
def _thirds(g, D):
    return {"gQ": g[:, :D], "gK": g[:, D:2 * D], "gV": g[:, 2 * D:]}


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_backward_under_the_float64_referee(heads, dh, monkeypatch):
    c = _case(heads, dh)
    qkv, g_out, ptr, D = c["qkv"], c["g_out"], c["ptr"], heads * dh
    what = f"attention backward heads={heads} dh={dh}"
    _, g32 = AO.autograd_backward(qkv, ptr, heads, g_out, torch.float32)
    _, g64 = AO.autograd_backward(qkv, ptr, heads, g_out, torch.float64)
    # the hand-written formulas are the autograd's
    hand = AO.backward(qkv.double(), ptr, heads, g_out.double())
    assert float((hand - g64).abs().max()) <= 1e-12 * float(g64.abs().max())
    spy = _Spy(monkeypatch)
    out, leaf = _hip_attention(qkv, ptr, heads, requires_grad=True)
    out.backward(g_out.to(DEV))
    assert spy.names == ["hscn_attention_fwd", "hscn_attention_bwd_q", "hscn_attention_bwd_kv"]
    got, o32, o64 = _thirds(leaf.grad, D), _thirds(g32, D), _thirds(g64, D)
    referee_all(got, o32, o64, what)
    g, j, _, _ = AO.largest_message(qkv, ptr, heads)
    _, d64 = AO.autograd_backward(qkv, ptr, heads, g_out, torch.float64, skip=(g, j))
    teeth(got, o32, o64, _thirds(d64, D), what + " [one key removed]")
    nd = _thirds(AO.backward(qkv.double(), ptr, heads, g_out.double(), no_delta=True), D)
    teeth(got, o32, o64, {"gQ": nd["gQ"], "gK": nd["gK"]}, what + " [no delta]")
    assert _flag() == 0


def test_no_backward_launch_when_qkv_needs_no_gradient(monkeypatch):
    c = _case(3, 8)
    spy = _Spy(monkeypatch)
    out, leaf = _hip_attention(c["qkv"], c["ptr"], 3, requires_grad=False)
    assert not out.requires_grad and out.grad_fn is None
    w = torch.ones_like(out, requires_grad=True)
    (out * w).sum().backward()
    assert leaf.grad is None and w.grad is not None
    assert spy.names == ["hscn_attention_fwd"]


def test_ptr32_on_another_device_is_refused_not_copied():
    c = _case(3, 8)
    with pytest.raises(RuntimeError, match="ptr32 is on cpu"):
        Fh.SelfAttentionFn.apply(c["qkv"].to(DEV), c["ptr"].to(torch.int32), max(c["sizes"]), 3)


# --------------------------------------------------------------------------- #
# 5. module pin: torch.nn.MultiheadAttention over a padded batch with key_padding_mask
# --------------------------------------------------------------------------- #
def _torch_mha(ref, x, ptr, gy, dtype):
    m = copy.deepcopy(ref).to(dtype)
    sizes = [int(v) for v in (ptr[1:] - ptr[:-1])]
    live = [(int(ptr[g]), n) for g, n in enumerate(sizes) if n]
    n_max = max(n for _, n in live)
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    rows = torch.cat([torch.arange(n) + b * n_max for b, (_, n) in enumerate(live)])
    dense = torch.zeros(len(live) * n_max, x.size(1), dtype=dtype).index_copy(0, rows, xx).view(len(live), n_max, -1)
    pad = torch.ones(len(live) * n_max, dtype=torch.bool)
    pad[rows] = False
    y, _ = m(dense, dense, dense, key_padding_mask=pad.view(len(live), n_max), need_weights=False)
    y = y.reshape(len(live) * n_max, -1)[rows]
    y.backward(gy.to(dtype))
    g = {"x.x": xx.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    return g, y.detach()


# (8, 64): embed_dim = 512, the top of the envelope -- both projections run through ``linear_wide`` in 80-column chunks
@pytest.mark.parametrize("heads,dh", HEAD_SHAPES + [(8, 64)])
def test_module_matches_torch_multihead_attention(heads, dh):
    c = _case(heads, dh)
    ptr, D = c["ptr"], heads * dh
    torch.manual_seed(heads + dh)
    ref = torch.nn.MultiheadAttention(D, heads, batch_first=True)
    with torch.no_grad():
        ref.in_proj_bias.normal_(std=0.1)
        ref.out_proj.bias.normal_(std=0.1)
    ours = MultiheadSelfAttention(D, heads).to(DEV)
    ours.load_state_dict(ref.state_dict(), strict=True)
    g = torch.Generator().manual_seed(7)
    N = int(ptr[-1])
    x, gy = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
    o32, y32 = _torch_mha(ref, x, ptr, gy, torch.float32)
    o64, y64 = _torch_mha(ref, x, ptr, gy, torch.float64)
    xd = x.to(DEV).requires_grad_(True)
    y = ours(xd, ptr32=ptr.to(torch.int32).to(DEV), max_nodes=max(c["sizes"]))
    y.backward(gy.to(DEV))
    what = f"MultiheadSelfAttention D={D} heads={heads}"
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    got = grads_of(ours, x=xd)
    assert set(got) == {"x.x", "p.in_proj_weight", "p.in_proj_bias", "p.out_proj.weight", "p.out_proj.bias"}
    referee_all(got, o32, o64, what)
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# 5b. linear_wide: a Linear whose weight is beyond hscn_linear_fwd's LDS image, at the widths of embed_dim = 512
# --------------------------------------------------------------------------- #
def _linear_ref(x, W, b, gy, dtype, drop=None):
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (x, W, b)]
    xx = leaves[0]
    if drop is not None:                                    # one input column left out of every sum
        keep = torch.ones(x.size(1), dtype=dtype)
        keep[drop] = 0
        xx = xx * keep
    y = xx @ leaves[1].t() + leaves[2]
    y.backward(gy.to(dtype))
    return dict(zip(("x.x", "x.W", "x.b"), (t.grad.detach().clone() for t in leaves))), y.detach()


# the packed projection [3D, D], the feed-forward pair [2D, D] / [D, 2D] and the square [D, D] of D = 512
@pytest.mark.parametrize("I,O", [(512, 1536), (512, 1024), (1024, 512), (512, 512)])
def test_linear_wide_forward_and_backward_at_embed_dim_512(I, O, monkeypatch):
    assert I * O * 4 > Fh.LINEAR_MAX_WEIGHT_BYTES
    g = torch.Generator().manual_seed(I + O)
    N = 37
    x, W = torch.randn(N, I, generator=g), torch.randn(O, I, generator=g) / I ** 0.5
    b, gy = 0.1 * torch.randn(O, generator=g), torch.randn(N, O, generator=g)
    o32, y32 = _linear_ref(x, W, b, gy, torch.float32)
    o64, y64 = _linear_ref(x, W, b, gy, torch.float64)
    d64, dy64 = _linear_ref(x, W, b, gy, torch.float64, drop=int(x.abs().sum(0).argmax()))
    spy = _Spy(monkeypatch)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, W, b)]
    y = Fh.linear_wide(*leaves)
    chunks = spy.names.count("hscn_linear_fwd")
    step = Fh.LINEAR_MAX_WEIGHT_BYTES // (4 * I) // 4 * 4
    assert chunks == -(-O // step) > 1 and y.shape == (N, O)
    y.backward(gy.to(DEV))
    got = dict(zip(("x.x", "x.W", "x.b"), (t.grad for t in leaves)))
    what = f"linear_wide {I} -> {O}"
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    teeth({"y": y}, {"y": y32}, {"y": y64}, {"y": dy64}, what)
    referee_all(got, o32, o64, what)
    teeth(got, o32, o64, {"x.x": d64["x.x"], "x.W": d64["x.W"]}, what)


# --------------------------------------------------------------------------- #
# 7. graph capture and the flag word
# --------------------------------------------------------------------------- #
def test_forward_and_backward_replay_from_a_captured_graph():
    heads, dh = 4, 24
    c = _case(heads, dh)
    ptr32 = c["ptr"].to(torch.int32).to(DEV)
    mn = max(c["sizes"])
    q = c["qkv"].to(DEV).requires_grad_(True)
    gd = c["g_out"].to(DEV)
    values = [torch.randn(c["qkv"].shape, generator=torch.Generator().manual_seed(s)).to(DEV) for s in (1, 2)]

    def run():
        out = Fh.SelfAttentionFn.apply(q, ptr32, mn, heads)
        return [out] + list(torch.autograd.grad(out, [q], gd))

    eager = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for v in values + values:
            with torch.no_grad():
                q.copy_(v)
            eager.append([t.clone() for t in run()])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for v, want in zip(values, eager[2:]):
        with torch.no_grad():
            q.copy_(v)
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "g_qkv"), outs, want):
            assert torch.equal(a, b), name
    assert not torch.equal(eager[2][0], eager[3][0])
    assert _flag() == 0


def test_an_understated_max_nodes_is_flagged_and_its_graphs_are_nan():
    heads, dh = 3, 8
    c = _case(heads, dh)
    qkv, g_out, ptr, sizes = c["qkv"], c["g_out"], c["ptr"], c["sizes"]
    T = int(_hip.lib().hscn_attention_tile())
    good, leaf = _hip_attention(qkv, ptr, heads, requires_grad=True)
    good.backward(g_out.to(DEV))
    assert _flag() == 0
    bad, leaf_b = _hip_attention(qkv, ptr, heads, max_nodes=T, requires_grad=True)      # two graphs have T + 1 nodes
    bad.backward(g_out.to(DEV))
    assert _flag() & Fh.ATTN_GRAPH_TOO_LARGE
    with pytest.raises(ValueError, match="max_nodes"):
        Fh.check_attention(DEV)
    assert _flag() == 0                                     # read and cleared
    over = torch.zeros(qkv.size(0), dtype=torch.bool)
    for g, n in enumerate(sizes):
        if n > T:
            over[int(ptr[g]):int(ptr[g + 1])] = True
    assert int(over.sum()) == sum(n for n in sizes if n > T) > 0
    for name, b, a in (("out", bad.detach(), good.detach()), ("g_qkv", leaf_b.grad, leaf.grad)):
        assert bool(torch.isnan(b[over.to(DEV)]).all()), name
        assert torch.equal(b[~over.to(DEV)], a[~over.to(DEV)]), name


def test_the_epoch_loops_report_a_graph_beyond_max_nodes():
    """``train.eval_epoch`` reads the attention flag word once per epoch (``GPS.check_flags``)."""
    from graph_hscn.train.train import eval_epoch
    graphs = make_dataset("peptides_func", 2, seed=0)
    b = Batch.from_data_list(graphs)
    torch.manual_seed(0)
    pm = GPS(9, LAYER_D, 10, 1, LAYER_HEADS, None, ACT_DICT["relu"]).to(DEV)
    assert np.isfinite(eval_epoch(0, None, [b], pm, "cross_entropy", None, "Test")[0])
    b.max_nodes = 1
    with pytest.raises(ValueError, match="max_nodes"):
        eval_epoch(0, None, [b], pm, "cross_entropy", None, "Test")
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# 6. GPSLayer and GPS against the CPU restatement of tests/gps_oracle.py
# --------------------------------------------------------------------------- #
# Gate condition (as tests/test_gpu_gine.py states it for its model case), asserted with no exclusion: every ReLU input
# (and GAT logit) of the float64 run lies farther from zero than 4 x the referee's own limit for that tensor,
# 2 max|f32 - f64| + 8 2^-23 max|f64|, so that no gate can differ between HIP, float32 and float64.  The seeds below
# were chosen on the CPU so that it holds.

LAYER_D, LAYER_HEADS, LAYER_DE = 16, 4, 3
LAYER_SIZES = [7, 1, 12, 0, 9]
LAYER_SEEDS = {None: 0, "gcn": 0, "gat": 0, "gine": 0}
# Two kinds of parameter gradient of the MODEL cases are sums the referee's scale says nothing about; they are named here
# with their reason and may, where the referee rejects them, pass by ``TermMagnitudes``' a-priori bound instead
# (``referee_all(cancelling=...)``), every other tensor passes the referee:
#   * ``attn.in_proj_bias``: its K third is sum_j gK_j = scale sum_i q_i (sum_j dS_ij) and sum_j dS_ij = 0 for every
#     row -- a shift of all keys' scores alike leaves the softmax unchanged -- so a third of the tensor is EXACTLY zero
#     in exact arithmetic and pure rounding residue of ~ N 2^-24 sum_j |gK_j| in any float32 evaluation, while the
#     referee's scale is the largest entry of the Q and V thirds;
#   * the last layer's ``norm2.bias`` at the graph level: behind the mean pool its gradient is sum_g g_pool[g], every
#     graph's term arriving as n_g equal parts g_pool[g] / n_g, of differing sign across graphs.  The float32
#     restatement's blocked sum of such parts is nearly exact (3.6 ulp of the tensor's scale on the case below), which
#     leaves the referee close to its 8-ulp floor, while an ordered float32 sum of N = 342 terms may carry N/2 ulp
#     (measured on the MI355X: 26 ulp, referee ratio 1.73).
# Teeth, for EVERY tensor so named (``bound_teeth``): against the float64 run with one term removed that changes the
# tensor most, the result must be rejected by the referee AND by that bound.  The removed terms: one key left out of
# every attention (it reaches ``in_proj_bias``; it does not reach the last ``norm2.bias``, whose gradient does not
# depend on the forward values) and, at graph level, one node left out of the pool's sum (it removes the part
# g_pool[0] / n_0 from ``norm2.bias``).
# Seeds: of the seeds 0..39 the one whose float64 run keeps the largest distance from its gates (a CPU-only choice).
# case -> dataset, graphs, F, C, local_conv, seed.  Four PascalVOC-SP-shaped graphs have ~1 800 nodes and ~10 000
# edges: with "gine" their 2 x 170 000 message pre-activations leave no seed that meets the gate condition, so the
# four-graph node-level case runs "gcn" and "gine" is refereed at node level on ONE such graph ("node-gine").
MODEL_CASES = {"graph": ("peptides_func", 4, 9, 10, "gine", 34), "node": ("pascalvoc_sp_node", 4, 14, 21, "gcn", 15),
               "node-gine": ("pascalvoc_sp_node", 1, 14, 21, "gine", 15),
               "link": ("pcqm_contact_link", 4, 9, 8, "gine", 18)}


def _level(case):
    return case.split("-")[0]


class _Terms(TermMagnitudes):
    """``TermMagnitudes`` plus the packed attention bias: d in_proj_bias = sum_r g_qkv[r]."""

    def __init__(self, model):
        super().__init__(model)
        self._attn = [(n, m) for n, m in model.named_modules() if isinstance(m, GPSO.AttentionRef)]
        for name, mod in self._attn:
            mod.term_hook = self._bias(name)

    def _bias(self, name):
        def term(qkv):
            if qkv.requires_grad:
                qkv.register_hook(lambda g: self._add(f"p.{name}.in_proj_bias", g.detach().abs().sum(0), g.shape[0]))
        return term

    def close(self):
        super().close()
        for _, mod in self._attn:
            mod.term_hook = None


def _check_gates(g32, g64, what):
    assert set(g32) == set(g64) and g64
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"{what} {tag}")


def _layer_inputs(seed):
    g = torch.Generator().manual_seed(3000 + seed)
    ptr = _ptr(LAYER_SIZES)
    N = int(ptr[-1])
    parts = []
    for k, n in enumerate(LAYER_SIZES):
        if n > 1:
            parts.append(torch.randint(0, n, (2, 3 * n), generator=g) + int(ptr[k]))
    ei = torch.cat(parts, 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()
    return (ptr, ei, torch.randn(N, LAYER_D, generator=g), torch.randn(ei.size(1), LAYER_DE, generator=g),
            torch.randn(N, LAYER_D, generator=g))


def _layer_run(ref, ptr, ei, x, ea, gy, dtype, skip=None):
    m = copy.deepcopy(ref).to(dtype)
    seen = {}
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    out = m(xx, ei, ptr, ea.to(dtype), skip)
    out.backward(gy.to(dtype))
    if m.local_conv == "gat":
        seen["gat logit"] = m.conv.last_logits.double()
    g = {"x.x": xx.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    return g, out.detach(), seen


def _layer_reference(local_conv, seed):
    """Everything of a layer case that is computed on the CPU (the seed search runs this alone)."""
    torch.manual_seed(seed)
    ref = GPSO.GPSLayerRef(LAYER_D, local_conv, LAYER_HEADS, "layer", LAYER_DE)
    inputs = _layer_inputs(seed)
    r32 = _layer_run(ref, *inputs, torch.float32)
    r64 = _layer_run(ref, *inputs, torch.float64)
    d64 = _layer_run(ref, *inputs, torch.float64, skip=(2, 0))
    return ref, inputs, r32, r64, d64


@pytest.mark.parametrize("local_conv", [None, "gcn", "gat", "gine"])
def test_gps_layer_under_the_float64_referee(local_conv):
    what = f"GPSLayer local_conv={local_conv}"
    ref, (ptr, ei, x, ea, gy), (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = \
        _layer_reference(local_conv, LAYER_SEEDS[local_conv])
    _check_gates(g32, g64, what)
    prod = GPSLayer(LAYER_D, local_conv, LAYER_HEADS, dropout=0.0, norm="layer", act="relu").to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    if local_conv == "gine":
        prod.conv.lin.materialize(LAYER_DE, xd)
    prod.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    y = prod(xd, ei.to(DEV), None, ea.to(DEV) if local_conv == "gine" else None,
             ptr32=ptr.to(torch.int32).to(DEV), max_nodes=max(LAYER_SIZES))
    y.backward(gy.to(DEV))
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    teeth({"y": y}, {"y": y32}, {"y": y64}, {"y": dy64}, what)
    got = grads_of(prod, x=xd)
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    assert {"x.x", "p.attn.in_proj_weight", "p.attn.out_proj.weight", "p.ff_linear1.weight"} <= set(reached)
    teeth(got, o32, o64, reached, what)
    assert _flag() == 0


def _model_batch(case):
    name, count, F, C, conv, seed = MODEL_CASES[case]
    graphs = make_dataset(name, count, seed=seed, edge_features=conv == "gine")
    return graphs, Batch.from_data_list(graphs), F, C, conv, seed


def _model_run(ref, b, gy, dtype, skip=None, terms=False, pool_skip=None):
    m = copy.deepcopy(ref).to(dtype)
    seen = {}
    if terms:
        seen = _Terms(m)
        pairs = b.edge_label_index if m.task_level == "link" else None
        ea = getattr(b, "edge_attr", None)
        m(b.x.to(dtype), b.edge_index, None if ea is None else ea.to(dtype), b.batch, b.ptr, int(b.num_graphs),
          pairs).backward(gy.to(dtype))
        seen.close()
        return seen
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
    pairs = b.edge_label_index if m.task_level == "link" else None
    ea = getattr(b, "edge_attr", None)
    out = m(b.x.to(dtype), b.edge_index, None if ea is None else ea.to(dtype), b.batch, b.ptr, int(b.num_graphs), pairs,
            skip, pool_skip)
    out.backward(gy.to(dtype))
    return {"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()}, out.detach(), seen


def _model_reference(case):
    """Everything of a model case that is computed on the CPU: the restatement, the batch, the cotangent, the float32
    and float64 runs and the float64 runs with one term removed (one key; at graph level also one pooled node)."""
    task_level = _level(case)
    graphs, b, F, C, conv, seed = _model_batch(case)
    torch.manual_seed(seed)
    ref = GPSO.GPSRef(F, LAYER_D, C, 2, LAYER_HEADS, conv, "layer", task_level,
                      int(b.edge_attr.size(1)) if conv == "gine" else None)
    rows = {"graph": (int(b.num_graphs), C), "node": (int(b.num_nodes), C)}.get(task_level) \
        or (int(b.edge_label_index.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))
    drops = [_model_run(ref, b, gy, torch.float64, skip=(0, 0))]
    if task_level == "graph":
        drops.append(_model_run(ref, b, gy, torch.float64, pool_skip=0))
    return ref, b, gy, _model_run(ref, b, gy, torch.float32), _model_run(ref, b, gy, torch.float64), drops


@pytest.mark.parametrize("case", sorted(MODEL_CASES))
def test_gps_model_under_the_float64_referee(case):
    from graph_hscn.train import batching
    task_level = _level(case)
    what = f"GPS {case} level"
    ref, b, gy, (o32, y32, g32), (o64, y64, g64), drops = _model_reference(case)
    d64, dy64 = drops[0][0], drops[0][1]
    F, C, conv = MODEL_CASES[case][2:5]
    assert len(g64) == 2 * (3 if conv == "gine" else 1) + 1
    _check_gates(g32, g64, what)
    pm = GPS(F, LAYER_D, C, 2, LAYER_HEADS, conv, ACT_DICT["relu"], 0.0, "layer", task_level).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    for layer in pm.layers:
        if conv == "gine":
            layer.conv.lin.materialize(int(b.edge_attr.size(1)), bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dy64}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values())
    terms = _model_run(ref, b, gy, torch.float64, terms=True)
    biases = [f"p.layers.{i}.attn.in_proj_bias" for i in range(2)]
    cancelling = biases + (["p.layers.1.norm2.bias"] if task_level == "graph" else [])
    referee_all(got, o32, o64, what, terms=terms, cancelling=cancelling)
    terms.bound_teeth(got, o32, o64, [d[0] for d in drops], cancelling, what)
    reached = most_changed(o64, [d64])
    assert {"p.node_encoder.weight", "p.layers.0.attn.in_proj_weight", "p.layers.1.attn.in_proj_weight"} <= set(reached)
    teeth(got, o32, o64, reached, what)
    Fh.check_attention(DEV)


@pytest.mark.parametrize("task_level", ["graph", "node", "link"])
def test_gps_trains_through_the_training_loop(task_level):
    """One ``train.train`` epoch of five steps on a fixed batch, with the task level's metric: the loss is finite and
    lower afterwards."""
    from types import SimpleNamespace

    from graph_hscn import metrics
    from graph_hscn.train.train import eval_epoch, train
    _, b, F, C, conv, seed = _model_batch(task_level)
    torch.manual_seed(seed)
    pm = GPS(F, LAYER_D, C, 2, LAYER_HEADS, conv, ACT_DICT["relu"], 0.0, "layer", task_level).to(DEV)
    loss_fn = "weighted_cross_entropy" if task_level == "node" else "cross_entropy"
    metric = {"graph": "ap", "node": "f1_macro", "link": "mrr"}[task_level]
    metric_fn = None if task_level == "link" else metrics.eval_hip(metric)
    extra = {"link_metric": metric} if task_level == "link" else {}
    before, perf = eval_epoch(0, None, [b], pm, loss_fn, metric_fn, "Test", **extra)
    assert np.isfinite(before) and 0.0 <= perf <= 1.0
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn=loss_fn, metric=metric, patience=10, min_delta=0.0)
    train(None, opt, cfg, [[b] * 5, [b], [b]], pm, metric_fn)
    after, perf = eval_epoch(1, None, [b], pm, loss_fn, metric_fn, "Test", **extra)
    assert np.isfinite(after) and after < before, (before, after)
    assert 0.0 <= perf <= 1.0
    Fh.check_attention(DEV)
