"""Shortest-path attention bias on the HIP path (csrc/spd.hip, csrc/attention.hip, nn/attention.py, nn/gps.py,
model/gps.py) against the plain-torch restatement of tests/attention_bias_oracle.py.

Buckets are integers: bit-exact against the oracle's BFS.  The operator, the module, the layer and the model go by
``referee_all`` (float32 and float64 restatements on the CPU as the two oracles) with ``teeth``; no new constants.

The table's gradient g_table[b, h] = sum over the pairs of bucket b of ds_ij is named in ``cancelling=``: every row's
ds_ij add up to zero (a shift of all logits of a row leaves the softmax unchanged), so with most pairs of a graph in a
few buckets the sum cancels and the referee's scale max|g_table| says little about its float32 residue.  Where the
referee rejects it, it may pass by ``TermMagnitudes``' a-priori bound 3 n 2^-24 sum|ds_ij| instead.  n is the longest
chain of additions a term goes through in the operator's documented order of summation (``_sum_depth``: a lane adds
its row's terms in key order, at most n_max of them; a tile adds its 64 lanes; the fold adds the B x tiles partials)
plus the lengths of the sums behind one term: the score (dh + 2), the row's softmax (n_max + 4), <g_out_i, v_j> (dh)
and delta_i (dh) -- at the model level the chain ``TermMagnitudes`` records.  Its teeth: against the float64 value with
the single largest ds_ij removed (the operator) or one key removed from every attention (the model) the result must
be rejected by the referee AND by that bound.

Shapes: one batch of random symmetric graphs of 1, 31, 32, 33, 64, 65 and 97 nodes (the bitset word, the chunk and the
tile edges, more than one tile), head shapes (1, 4), (4, 8), (2, 64), max_dist = 5 (six buckets)."""
import copy

import numpy as np
import pytest
import torch

import tests.test_gpu_attention as TA
from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import Batch, Data
from graph_hscn.model.gps import GPS
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import MultiheadSelfAttention
from graph_hscn.nn.gps import GPSLayer
from tests import attention_bias_oracle as BO
from tests import gps_oracle as GPSO
from tests.helpers import DEV, TermMagnitudes, grads_of, most_changed, referee_all, teeth

pytestmark = pytest.mark.gpu

HEAD_SHAPES = [(1, 4), (4, 8), (2, 64)]
SIZES = [1, 31, 32, 33, 64, 65, 97]
MAX_DIST = 5


class _Spy:
    """Names of the C-ABI entries issued through nn.functional while active."""

    def __init__(self, monkeypatch):
        self.names = []
        real = Fh.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(Fh, "call", call)


def _sum_depth(num_graphs, max_nodes):
    """The longest chain of additions behind one entry of the table's gradient: keys of a row, lanes of a tile, tiles."""
    tile = int(_hip.lib().hscn_attention_tile())
    return max_nodes + tile + num_graphs * max(1, -(-max_nodes // tile))


def _spd_flag():
    return int(Fh.spd_flags(DEV).item())


def _attn_flag():
    return int(Fh.attention_flags(DEV).item())


def _batch_of(graphs):
    return Batch.from_data_list([Data(x=torch.zeros(n, 1), edge_index=ei) for n, ei in graphs])


def _to_dev(b):
    """On the device the way the training loop moves a batch (the node counts stay on the host beside it)."""
    from graph_hscn.train import batching
    return batching.to_device(None, b, DEV)


def _device_spd(buckets, max_dist, max_nodes):
    """The oracle's matrices in the operator's layout on the device (the operator tests do not lean on the bucket kernel)."""
    data, sptr = BO.flat(buckets)
    return Fh.SPDBuckets(data.to(DEV), sptr.to(DEV), max_dist, max_nodes)


# --------------------------------------------------------------------------- #
# 1. the bucket kernel, bit for bit
# --------------------------------------------------------------------------- #
_EDGE = {}


def _edge_case():
    if not _EDGE:
        graphs = BO.edge_case_graphs()
        ei, ptr, eptr = BO.collate(graphs)
        _EDGE.update(graphs=graphs, ei=ei, ptr=ptr, eptr=eptr, batch=_to_dev(_batch_of(graphs)))
    return _EDGE


@pytest.mark.parametrize("max_dist", [1, MAX_DIST, 63])
def test_buckets_equal_the_oracle_bfs_on_the_edge_case_batch(max_dist):
    c = _edge_case()
    want, want_ptr = BO.flat(BO.bfs_buckets(c["ei"], c["ptr"], max_dist, c["eptr"]))
    spd = Fh.shortest_path_buckets(c["batch"], max_dist)
    assert spd.bucket.dtype == torch.uint8 and spd.spd_ptr.dtype == torch.int64
    assert (spd.max_dist, spd.max_nodes, spd.num_buckets) == (max_dist, 97, max_dist + 1)
    assert torch.equal(spd.spd_ptr.cpu(), want_ptr)
    assert torch.equal(spd.bucket.cpu(), want)
    assert int(spd.bucket.max()) == max_dist                  # the cap is reached (disconnected pairs)
    again = Fh.shortest_path_buckets(c["batch"], max_dist)
    assert torch.equal(again.bucket, spd.bucket)
    assert _spd_flag() == 0
    Fh.check_spd(DEV)


def test_a_graph_has_the_same_buckets_wherever_it_stands():
    graphs = BO.edge_case_graphs()
    first, last = _to_dev(_batch_of(graphs[-1:] + graphs[:4])), _to_dev(_batch_of(graphs[2:]))
    a = Fh.shortest_path_buckets(first, MAX_DIST)
    b = Fh.shortest_path_buckets(last, MAX_DIST)
    n = graphs[-1][0]
    assert int(a.spd_ptr[1]) == n * n and int(b.spd_ptr[-1] - b.spd_ptr[-2]) == n * n
    assert torch.equal(a.bucket[:n * n], b.bucket[-n * n:])
    assert torch.equal(a.bucket[:n * n].cpu(), BO.bfs_buckets(graphs[-1][1], [0, n], MAX_DIST)[0].reshape(-1))
    assert _spd_flag() == 0


def test_an_edge_outside_its_graph_is_flagged_and_skipped():
    c = _edge_case()
    ei = c["ei"].clone()
    k = int(c["eptr"][4]) + 3                                 # an edge of the 12-node path ...
    ei[1, k] = int(c["ptr"][6])                               # ... now ends in another graph
    want = BO.flat(BO.bfs_buckets(ei, c["ptr"], MAX_DIST, c["eptr"]))[0]
    assert not torch.equal(want, BO.flat(BO.bfs_buckets(c["ei"], c["ptr"], MAX_DIST, c["eptr"]))[0])
    b = c["batch"]
    sizes = [n for n, _ in c["graphs"]]
    spd = Fh.shortest_path_buckets((ei.to(DEV), b.ptr32, b.eptr32, b.max_nodes), MAX_DIST, sizes=sizes)
    assert torch.equal(spd.bucket.cpu(), want)
    assert _spd_flag() == Fh.SPD_EDGE_OUT_OF_RANGE
    with pytest.raises(ValueError, match="outside its graph"):
        Fh.check_spd(DEV)
    assert _spd_flag() == 0                                   # read and cleared


def test_an_understated_max_nodes_is_flagged_and_its_graphs_are_all_max_dist():
    c = _edge_case()
    b = c["batch"]
    sizes = [n for n, _ in c["graphs"]]
    want = BO.bfs_buckets(c["ei"], c["ptr"], MAX_DIST, c["eptr"])
    want = [m if m.size(0) <= 64 else torch.full_like(m, MAX_DIST) for m in want]
    assert sum(m.size(0) > 64 for m in want) == 2
    spd = Fh.shortest_path_buckets((b.edge_index, b.ptr32, b.eptr32, 64), MAX_DIST, sizes=sizes)
    assert torch.equal(spd.bucket.cpu(), BO.flat(want)[0])
    assert _spd_flag() == Fh.SPD_GRAPH_TOO_LARGE
    with pytest.raises(ValueError, match="max_nodes"):
        Fh.check_spd(DEV)
    assert _spd_flag() == 0


def test_a_cycle_at_the_largest_supported_size_is_exact():
    n = max(k for k in range(512, 1025) if Fh.spd_supported(k, 63))
    assert not Fh.spd_supported(n + 1, 63)
    idx = torch.arange(n)
    e = torch.stack([idx, (idx + 1) % n])
    ei = torch.cat([e, e.flip(0)], 1)
    spd = Fh.shortest_path_buckets(_to_dev(_batch_of([(n, ei)])), 63)
    gap = (idx[:, None] - idx[None, :]).abs()
    want = torch.minimum(gap, n - gap).clamp(max=63).to(torch.uint8)
    assert torch.equal(spd.bucket.cpu().view(n, n), want)
    assert torch.equal(want, BO.bfs_buckets(ei, [0, n], 63)[0])
    assert _spd_flag() == 0


# --------------------------------------------------------------------------- #
# 2. the biased operator
# --------------------------------------------------------------------------- #
_CASES = {}


def _case(heads, dh):
    """Inputs and the two CPU runs of one head shape, computed once and shared (never modified)."""
    key = (heads, dh)
    if key not in _CASES:
        graphs = [(n, BO.random_symmetric(n, 2000 + n)) for n in SIZES]
        ei, ptr, eptr = BO.collate(graphs)
        buckets = BO.bfs_buckets(ei, ptr, MAX_DIST, eptr)
        g = torch.Generator().manual_seed(100 * heads + dh)
        N, D = int(ptr[-1]), heads * dh
        qkv = torch.randn(N, 3 * D, generator=g)
        g_out = torch.randn(N, D, generator=g)
        table = torch.randn(MAX_DIST + 1, heads, generator=g)
        _CASES[key] = dict(graphs=graphs, ptr=ptr, buckets=buckets, qkv=qkv, g_out=g_out, table=table,
                           o32=BO.run(qkv, table, buckets, ptr, heads, g_out, torch.float32),
                           o64=BO.run(qkv, table, buckets, ptr, heads, g_out, torch.float64))
    return _CASES[key]


def _hip_run(c, heads, table=None, buckets=None, ptr=None, qkv=None, g_out=None, need=(True, True)):
    """{"out", "gQ", "gK", "gV", "g_table"} of the operator on the device (a gradient not asked for: None)."""
    ptr = c["ptr"] if ptr is None else ptr
    buckets = c["buckets"] if buckets is None else buckets
    sizes = ptr[1:] - ptr[:-1]
    mn = int(sizes.max())
    q = (c["qkv"] if qkv is None else qkv).to(DEV).requires_grad_(need[0])
    t = (c["table"] if table is None else table).to(DEV).requires_grad_(need[1])
    out = Fh.BiasedSelfAttentionFn.apply(q, t, _device_spd(buckets, MAX_DIST, mn), ptr.to(torch.int32).to(DEV), mn, heads)
    if any(need):
        out.backward((c["g_out"] if g_out is None else g_out).to(DEV))
    D = q.size(1) // 3
    gq = q.grad
    return {"out": out.detach(), "gQ": None if gq is None else gq[:, :D], "gK": None if gq is None else gq[:, D:2 * D],
            "gV": None if gq is None else gq[:, 2 * D:], "g_table": t.grad}


def _table_terms(c, heads, dh):
    """(TermMagnitudes holding g_table's a-priori terms, the float64 g_table with its largest pair term removed)."""
    mag, count, gt, (val, b, h) = BO.table_terms(c["qkv"], c["table"], c["buckets"], c["ptr"], heads, c["g_out"])
    assert float((gt - c["o64"]["g_table"]).abs().max()) <= 1e-11 * float(mag.max())     # the formula is autograd's
    terms = TermMagnitudes(torch.nn.Module(), chain_extra=(dh + 2) + (max(SIZES) + 4) + dh + dh)
    assert int(count.sum()) == sum(n * n for n in SIZES)
    terms._add("g_table", mag, _sum_depth(len(SIZES), max(SIZES)))
    dropped = c["o64"]["g_table"].clone()
    dropped[b, h] -= val
    return terms, dropped


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_operator_under_the_float64_referee_with_teeth(heads, dh):
    c = _case(heads, dh)
    what = f"biased attention heads={heads} dh={dh}"
    got = _hip_run(c, heads)
    assert got["out"].shape == (c["qkv"].size(0), heads * dh) and got["g_table"].shape == (MAX_DIST + 1, heads)
    terms, dropped_table = _table_terms(c, heads, dh)
    referee_all(got, c["o32"], c["o64"], what, terms=terms, cancelling=["g_table"])
    # one bucket's bias zeroed (the neighbours'): every tensor the logits reach must notice
    zeroed = c["table"].clone()
    zeroed[1] = 0.0
    z64 = BO.run(c["qkv"], zeroed, c["buckets"], c["ptr"], heads, c["g_out"], torch.float64)
    teeth(got, c["o32"], c["o64"], {k: z64[k] for k in ("out", "gQ", "gK", "gV")}, what + " [bucket 1 zeroed]")
    # the table's gradient with its single largest pair term removed: rejected by the referee and by the bound
    d64 = dict(c["o64"], g_table=dropped_table)
    terms.bound_teeth(got, c["o32"], c["o64"], [d64], ["g_table"], what)
    assert _attn_flag() == 0


def _lse_of(c, heads, table):
    q = c["qkv"].to(DEV).contiguous()
    N, D = q.size(0), q.size(1) // 3
    mn = max(SIZES)
    ptr32 = c["ptr"].to(torch.int32).to(DEV)
    out, lse = torch.empty(N, D, device=DEV), torch.empty(N, heads, device=DEV)
    flag = _hip.ptr(Fh.attention_flags(DEV))
    if table is None:
        _hip.call("hscn_attention_fwd", _hip.ptr(q), _hip.ptr(ptr32), N, len(SIZES), mn, heads, D // heads,
                  _hip.ptr(out), _hip.ptr(lse), flag, _hip.stream())
    else:
        spd, t = _device_spd(c["buckets"], MAX_DIST, mn), table.to(DEV)
        _hip.call("hscn_attention_bias_fwd", _hip.ptr(q), _hip.ptr(t), _hip.ptr(spd.bucket), _hip.ptr(spd.spd_ptr),
                  _hip.ptr(ptr32), N, len(SIZES), spd.bucket.numel(), mn, heads, D // heads, t.size(0), _hip.ptr(out),
                  _hip.ptr(lse), flag, _hip.stream())
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_a_zero_table_gives_the_bits_of_the_unbiased_operator(heads, dh):
    c = _case(heads, dh)
    zero = torch.zeros(MAX_DIST + 1, heads)
    got = _hip_run(c, heads, table=zero)
    q = c["qkv"].to(DEV).requires_grad_(True)
    out = Fh.SelfAttentionFn.apply(q, c["ptr"].to(torch.int32).to(DEV), max(SIZES), heads)
    out.backward(c["g_out"].to(DEV))
    D = heads * dh
    assert torch.equal(got["out"], out.detach())
    assert torch.equal(torch.cat([got["gQ"], got["gK"], got["gV"]], 1), q.grad)
    o_b, lse_b = _lse_of(c, heads, zero)
    o_u, lse_u = _lse_of(c, heads, None)
    assert torch.equal(lse_b, lse_u) and torch.equal(o_b, o_u) and torch.equal(o_b, got["out"])
    assert D == q.grad.size(1) // 3 and _attn_flag() == 0


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_two_runs_agree_bit_for_bit_and_a_graph_does_not_depend_on_its_place(heads, dh):
    c = _case(heads, dh)
    a, b = _hip_run(c, heads), _hip_run(c, heads)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the last graph alone, and behind other rows
    n = SIZES[-1]
    s = int(c["ptr"][-2])
    alone = _hip_run(c, heads, buckets=c["buckets"][-1:], ptr=torch.tensor([0, n]), qkv=c["qkv"][s:], g_out=c["g_out"][s:])
    other = c["qkv"].clone()
    other[:s] = torch.randn(s, other.size(1), generator=torch.Generator().manual_seed(5))
    changed = _hip_run(c, heads, qkv=other)
    for k in ("out", "gQ", "gK", "gV"):
        assert torch.equal(a[k][s:], alone[k]), k
        assert torch.equal(a[k][s:], changed[k][s:]), k
        assert not torch.equal(a[k][:s], changed[k][:s]), k
    assert _attn_flag() == 0


def test_backward_launches_only_for_the_inputs_that_need_a_gradient(monkeypatch):
    heads, dh = 4, 8
    c = _case(heads, dh)
    both = _hip_run(c, heads)
    spy = _Spy(monkeypatch)
    only_q = _hip_run(c, heads, need=(True, False))
    assert spy.names == ["hscn_attention_bias_fwd", "hscn_attention_bias_bwd_q", "hscn_attention_bias_bwd_kv"]
    assert only_q["g_table"] is None
    for k in ("gQ", "gK", "gV"):
        assert torch.equal(only_q[k], both[k]), k
    spy.names.clear()
    only_t = _hip_run(c, heads, need=(False, True))
    assert spy.names == ["hscn_attention_bias_fwd", "hscn_attention_bias_bwd_q"]
    assert only_t["gQ"] is None and torch.equal(only_t["g_table"], both["g_table"])
    spy.names.clear()
    none = _hip_run(c, heads, need=(False, False))
    assert spy.names == ["hscn_attention_bias_fwd"] and none["g_table"] is None and none["gQ"] is None
    assert torch.equal(none["out"], both["out"])


def test_forward_and_backward_replay_from_a_captured_graph():
    heads, dh = 4, 8
    c = _case(heads, dh)
    mn = max(SIZES)
    ptr32 = c["ptr"].to(torch.int32).to(DEV)
    spd = _device_spd(c["buckets"], MAX_DIST, mn)
    q = c["qkv"].to(DEV).requires_grad_(True)
    t = c["table"].to(DEV).requires_grad_(True)
    gd = c["g_out"].to(DEV)
    values = [(torch.randn(c["qkv"].shape, generator=torch.Generator().manual_seed(s)).to(DEV),
               torch.randn(c["table"].shape, generator=torch.Generator().manual_seed(s + 10)).to(DEV)) for s in (1, 2)]

    def run():
        out = Fh.BiasedSelfAttentionFn.apply(q, t, spd, ptr32, mn, heads)
        return [out] + list(torch.autograd.grad(out, [q, t], gd))

    eager = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for vq, vt in values + values:
            with torch.no_grad():
                q.copy_(vq)
                t.copy_(vt)
            eager.append([x.clone() for x in run()])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for (vq, vt), want in zip(values, eager[2:]):
        with torch.no_grad():
            q.copy_(vq)
            t.copy_(vt)
        for x in outs:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "g_qkv", "g_table"), outs, want):
            assert torch.equal(a, b), name
    assert not torch.equal(eager[2][2], eager[3][2])
    assert _attn_flag() == 0


def test_buckets_of_another_batch_are_flagged_not_read():
    heads, dh = 4, 8
    c = _case(heads, dh)
    mn = max(SIZES)
    short = Fh.SPDBuckets(torch.zeros(100, dtype=torch.uint8, device=DEV), _device_spd(c["buckets"], MAX_DIST, mn).spd_ptr,
                          MAX_DIST, mn)
    out = Fh.BiasedSelfAttentionFn.apply(c["qkv"].to(DEV), c["table"].to(DEV), short, c["ptr"].to(torch.int32).to(DEV),
                                         mn, heads)
    assert bool(torch.isnan(out[1:]).all()) and not bool(torch.isnan(out[:1]).any())     # the one-node graph fits
    assert _attn_flag() == Fh.ATTN_BUCKETS_OUT_OF_RANGE
    with pytest.raises(ValueError, match="bucket range"):
        Fh.check_attention(DEV)
    assert _attn_flag() == 0


# --------------------------------------------------------------------------- #
# 3. the module against torch.nn.MultiheadAttention with a float attn_mask per graph
# --------------------------------------------------------------------------- #
def _torch_mha(ref, table, buckets, x, ptr, gy, dtype):
    m = copy.deepcopy(ref).to(dtype)
    t = table.detach().clone().to(dtype).requires_grad_(True)
    xx = x.detach().clone().to(dtype).requires_grad_(True)
    ys = []
    for g in range(len(ptr) - 1):
        s, e = int(ptr[g]), int(ptr[g + 1])
        if e > s:
            mask = t[buckets[g].long()].permute(2, 0, 1)              # [heads, n, n], added to the logits
            ys.append(m(xx[s:e][None], xx[s:e][None], xx[s:e][None], attn_mask=mask, need_weights=False)[0][0])
    y = torch.cat(ys)
    y.backward(gy.to(dtype))
    g = {"x.x": xx.grad.detach().clone(), "p.spd_bias.weight": t.grad.detach().clone()}
    g.update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    return g, y.detach()


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_module_matches_torch_multihead_attention_with_a_float_mask(heads, dh):
    c = _case(heads, dh)
    ptr, D, K = c["ptr"], heads * dh, MAX_DIST + 1
    torch.manual_seed(heads + dh)
    ref = torch.nn.MultiheadAttention(D, heads, batch_first=True)
    with torch.no_grad():
        ref.in_proj_bias.normal_(std=0.1)
        ref.out_proj.bias.normal_(std=0.1)
    ours = MultiheadSelfAttention(D, heads, spd_buckets=K).to(DEV)
    state = dict(ref.state_dict())
    state["spd_bias.weight"] = c["table"]
    ours.load_state_dict(state, strict=True)
    g = torch.Generator().manual_seed(7)
    N = int(ptr[-1])
    x, gy = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
    o32, y32 = _torch_mha(ref, c["table"], c["buckets"], x, ptr, gy, torch.float32)
    o64, y64 = _torch_mha(ref, c["table"], c["buckets"], x, ptr, gy, torch.float64)
    z64, zy64 = _torch_mha(ref, torch.zeros_like(c["table"]), c["buckets"], x, ptr, gy, torch.float64)
    xd = x.to(DEV).requires_grad_(True)
    y = ours(xd, ptr32=ptr.to(torch.int32).to(DEV), max_nodes=max(SIZES), spd=_device_spd(c["buckets"], MAX_DIST, max(SIZES)))
    y.backward(gy.to(DEV))
    what = f"MultiheadSelfAttention(spd_buckets={K}) D={D} heads={heads}"
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    teeth({"y": y}, {"y": y32}, {"y": y64}, {"y": zy64}, what + " [no bias]")
    got = grads_of(ours, x=xd)
    assert set(got) == {"x.x", "p.in_proj_weight", "p.in_proj_bias", "p.out_proj.weight", "p.out_proj.bias",
                        "p.spd_bias.weight"}
    referee_all(got, o32, o64, what)
    teeth(got, o32, o64, {k: z64[k] for k in ("x.x", "p.in_proj_weight", "p.out_proj.weight")}, what + " [no bias]")
    assert _attn_flag() == 0


# --------------------------------------------------------------------------- #
# 4. GPSLayer and GPS against tests/gps_oracle.py with the biased attention put in
# --------------------------------------------------------------------------- #
LAYER_MAX_DIST = 4
# Seeds chosen on the CPU so that the gate condition of tests/test_gpu_attention.py holds (every ReLU input of the
# float64 run farther from zero than 4 x the referee's own limit for that tensor): _check_gates asserts it.
LAYER_SEEDS = {None: 0, "gine": 0}
MODEL_SEED = 34


class _Terms(TA._Terms):
    """tests/test_gpu_attention.py's term magnitudes plus the bias tables': d spd_bias.weight[b, h] is the sum of the
    gathered bias tensor's cotangent (ds_ij) over the pairs of bucket b; ``rows`` = ``_sum_depth`` of the batch."""

    def __init__(self, model, depth):
        super().__init__(model)
        self._tables = []
        for name, mod in self._attn:
            key = f"p.{name}.spd_bias.weight"
            self._tables.append(key)
            self.rows[key] = int(depth)
            mod.bias_hook = self._table(key, tuple(mod.spd_bias.weight.shape))

    def _table(self, key, shape):
        def term(bias, bucket):
            flat = bucket.reshape(-1)

            def back(g):
                mag = torch.zeros(shape, dtype=g.dtype).index_add_(0, flat, g.detach().abs().reshape(-1, shape[1]))
                self._add(key, mag, 0)
            if bias.requires_grad:
                bias.register_hook(back)
        return term

    def close(self):
        super().close()
        for _, mod in self._attn:
            mod.bias_hook = None


def _layer_reference(local_conv, seed):
    torch.manual_seed(seed)
    ref = GPSO.GPSLayerRef(TA.LAYER_D, local_conv, TA.LAYER_HEADS, "layer", TA.LAYER_DE)
    inputs = TA._layer_inputs(seed)
    ptr, ei = inputs[0], inputs[1]
    buckets = BO.bfs_buckets(ei, ptr, LAYER_MAX_DIST)
    BO.with_spd(ref, LAYER_MAX_DIST + 1, buckets)
    r32 = TA._layer_run(ref, *inputs, torch.float32)
    r64 = TA._layer_run(ref, *inputs, torch.float64)
    d64 = TA._layer_run(ref, *inputs, torch.float64, skip=(2, 0))
    return ref, inputs, buckets, r32, r64, d64


@pytest.mark.parametrize("local_conv", [None, "gine"])
def test_gps_layer_with_the_bias_under_the_float64_referee(local_conv):
    what = f"GPSLayer(spd_buckets={LAYER_MAX_DIST + 1}) local_conv={local_conv}"
    ref, (ptr, ei, x, ea, gy), buckets, (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = \
        _layer_reference(local_conv, LAYER_SEEDS[local_conv])
    TA._check_gates(g32, g64, what)
    prod = GPSLayer(TA.LAYER_D, local_conv, TA.LAYER_HEADS, dropout=0.0, norm="layer", act="relu",
                    spd_buckets=LAYER_MAX_DIST + 1).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    if local_conv == "gine":
        prod.conv.lin.materialize(TA.LAYER_DE, xd)
    prod.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    mn = max(TA.LAYER_SIZES)
    y = prod(xd, ei.to(DEV), None, ea.to(DEV) if local_conv == "gine" else None, ptr32=ptr.to(torch.int32).to(DEV),
             max_nodes=mn, spd=_device_spd(buckets, LAYER_MAX_DIST, mn))
    y.backward(gy.to(DEV))
    referee_all({"y": y}, {"y": y32}, {"y": y64}, what)
    teeth({"y": y}, {"y": y32}, {"y": y64}, {"y": dy64}, what)
    got = grads_of(prod, x=xd)
    assert "p.attn.spd_bias.weight" in got and got["p.attn.spd_bias.weight"] is not None
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    assert {"x.x", "p.attn.in_proj_weight", "p.attn.spd_bias.weight", "p.ff_linear1.weight"} <= set(reached)
    teeth(got, o32, o64, reached, what)
    assert _attn_flag() == 0


def _model_reference():
    graphs, b, F, C, conv, _ = TA._model_batch("graph")
    torch.manual_seed(MODEL_SEED)
    ref = GPSO.GPSRef(F, TA.LAYER_D, C, 2, TA.LAYER_HEADS, conv, "layer", "graph", int(b.edge_attr.size(1)))
    buckets = BO.bfs_buckets(b.edge_index, b.ptr, LAYER_MAX_DIST, b.eptr32)
    BO.with_spd(ref, LAYER_MAX_DIST + 1, buckets)
    gy = torch.randn(int(b.num_graphs), C, generator=torch.Generator().manual_seed(1))
    drops = [TA._model_run(ref, b, gy, torch.float64, skip=(0, 0)), TA._model_run(ref, b, gy, torch.float64, pool_skip=0)]
    return ref, b, F, C, conv, gy, TA._model_run(ref, b, gy, torch.float32), TA._model_run(ref, b, gy, torch.float64), drops


def _model_terms(ref, b, gy):
    m = copy.deepcopy(ref).double()
    seen = _Terms(m, _sum_depth(int(b.num_graphs), int(b.max_nodes)))
    m(b.x.double(), b.edge_index, b.edge_attr.double(), b.batch, b.ptr, int(b.num_graphs), None).backward(gy.double())
    seen.close()
    return seen


def test_gps_model_with_the_bias_under_the_float64_referee(monkeypatch):
    from graph_hscn.train import batching
    what = "GPS(attn_bias='spd') graph level"
    ref, b, F, C, conv, gy, (o32, y32, g32), (o64, y64, g64), drops = _model_reference()
    assert int(b.num_graphs) == 4
    TA._check_gates(g32, g64, what)
    pm = GPS(F, TA.LAYER_D, C, 2, TA.LAYER_HEADS, conv, ACT_DICT["relu"], 0.0, "layer", "graph", attn_bias="spd",
             spd_max_dist=LAYER_MAX_DIST).to(DEV)
    bd = batching.to_device(pm, b, DEV)
    for layer in pm.layers:
        layer.conv.lin.materialize(int(b.edge_attr.size(1)), bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    spy = _Spy(monkeypatch)
    pred = pm(bd)
    assert spy.names.count("hscn_spd_buckets") == 1 and spy.names.count("hscn_attention_bias_fwd") == 2
    pred.backward(gy.to(DEV))
    # the buckets are the oracle's, and a second forward -- also of a fresh device copy of the same host batch --
    # finds them on the batch
    spd = bd._spd_cache[(LAYER_MAX_DIST, str(bd.ptr32.device))]
    assert torch.equal(spd.bucket.cpu(), BO.flat(BO.bfs_buckets(b.edge_index, b.ptr, LAYER_MAX_DIST, b.eptr32))[0])
    spy.names.clear()
    with torch.no_grad():
        again = pm(bd)
        moved = pm(batching.to_device(pm, b, DEV))
    assert "hscn_spd_buckets" not in spy.names and torch.equal(again, pred) and torch.equal(moved, pred)
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": drops[0][1]}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values())
    terms = _model_terms(ref, b, gy)
    # in_proj_bias and the last norm2.bias: the reasons of tests/test_gpu_attention.py; the tables: every row's ds_ij
    # add up to zero and with max_dist = 4 nearly all pairs of these chain-like graphs share the last bucket, whose sum
    # of ~36 000 terms cancels to 1/30 of sum|ds_ij| (this file's docstring)
    tables = [f"p.layers.{i}.attn.spd_bias.weight" for i in range(2)]
    cancelling = [f"p.layers.{i}.attn.in_proj_bias" for i in range(2)] + ["p.layers.1.norm2.bias"] + tables
    assert set(tables) <= set(got)
    referee_all(got, o32, o64, what, terms=terms, cancelling=cancelling)
    terms.bound_teeth(got, o32, o64, [d[0] for d in drops], cancelling, what)
    reached = most_changed(o64, [drops[0][0]])
    assert {"p.node_encoder.weight", "p.layers.0.attn.in_proj_weight", "p.layers.0.attn.spd_bias.weight"} <= set(reached)
    teeth(got, o32, o64, {k: v for k, v in reached.items() if k not in cancelling}, what)
    pm.check_flags()


@pytest.mark.parametrize("task_level", ["graph", "node"])
def test_gps_with_the_bias_trains_through_the_training_loop(task_level):
    from types import SimpleNamespace

    from graph_hscn import metrics
    from graph_hscn.train.train import eval_epoch, train
    _, b, F, C, conv, seed = TA._model_batch(task_level)
    torch.manual_seed(seed)
    pm = GPS(F, TA.LAYER_D, C, 2, TA.LAYER_HEADS, conv, ACT_DICT["relu"], 0.0, "layer", task_level, attn_bias="spd",
             spd_max_dist=8).to(DEV)
    before = [layer.attn.spd_bias.weight.detach().clone() for layer in pm.layers]
    loss_fn = "weighted_cross_entropy" if task_level == "node" else "cross_entropy"
    metric_fn = metrics.eval_hip({"graph": "ap", "node": "f1_macro"}[task_level])
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn=loss_fn, metric={"graph": "ap", "node": "f1_macro"}[task_level],
                          patience=10, min_delta=0.0)
    train(None, opt, cfg, [[b] * 3, [b], [b]], pm, metric_fn)
    after, perf = eval_epoch(1, None, [b], pm, loss_fn, metric_fn, "Test")
    assert np.isfinite(after) and 0.0 <= perf <= 1.0
    for w0, layer in zip(before, pm.layers):
        w = layer.attn.spd_bias.weight.detach()
        assert bool(torch.isfinite(w).all()) and not torch.equal(w, w0)
    assert len(b._spd_cache) == 1                             # one build for the whole run: the host batch keeps it
    pm.check_flags()
