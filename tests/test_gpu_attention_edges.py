"""The attention kernel family (csrc/attention.hip) at its tile, fold and bucket edges, against the plain-torch
restatements of tests/attention_oracle.py and tests/attention_bias_oracle.py.

Tolerances are those of tests/test_gpu_attention.py and tests/test_gpu_attention_bias.py, no new constants: the plain
forward by ``check_f64`` (n_out = n + 4 + 2 (dh + 2) a), lse by ``f64_close`` (n + dh + 6, a + 1 + |lse64|), every
gradient and the biased forward by ``referee_all`` with ``teeth``; g_table is named in ``cancelling=`` with a
``TermMagnitudes`` of depth ``_sum_depth(B, max_nodes)`` + (dh + 2) + (n_max + 4) + dh + dh and ``bound_teeth`` against
the float64 value with the single largest ds_ij removed.  B and n_max are the case's, max_nodes the value handed to the
operator.  T = hscn_attention_tile(), C = hscn_attention_chunk().  The oracle gathers table[bucket] directly, so it is
given clamp(max = nb - 1) of a bucket matrix wherever the device gets raw bytes >= nb.

What each section is about, in csrc/attention.hip:
  1. the dispatch ladder ``HSCN_ATTN_CASE(4) .. HSCN_ATTN_CASE(64)`` of ``launch``: forward, ``k_attn_bwd_q`` and
     ``k_attn_bwd_kv`` of AttnArgs and BiasArgs at all 16 widths, and ``attn_supported`` at its edges;
  2. ``row0 = t * AT_TILE`` with t >= 2 (``graph_range``), more than four chunks of AT_CHUNK keys, and tiles with
     ``row0 >= n``: the early ``return`` of the three kernels and the zero partial ``write_partial(A, h, 0.f)`` that
     ``k_bias_fold`` then adds;
  3. ``k_bias_fold``: the unrolled loop over blocks of ``AB_FOLD_AHEAD`` = 32 partials with 31, 32, 33 and 65 tiles in
     the launch, ``AB_FOLD_THREADS`` = 64 with heads * nb = 64, 66 and 68 (``blockIdx.x`` > 0, the ``idx >= hb`` guard),
     and the [tile, head, bucket] -> [bucket, head] transposition;
  4. ``AB_MAX_BUCKETS`` = 64 and the dynamic bins ``bins[nb][64]`` (16 KB at nb = 64 beside the static arrays of
     dh = 64), nb = 1, and the two bucket clamps: ``staged_bucket`` (forward, bwd_q) and ``b < A.nb ? b : A.nb - 1``
     in ``k_attn_bwd_kv``;
  5. the online softmax: ``if (c0 == 0) m = cmax; else if (cmax > m)`` with its rescale by ``expf(m - cmax)``, and the
     backward's ``expf(s - lse)``, on rows whose maximum sits in the last chunk or in the first with later terms
     underflowing;
  6. the three refusal blocks of the backward kernels (``if (const int why = refusal(...))`` in ``k_attn_bwd_q``,
     ``k_attn_bwd_kv`` and, for the table, ``write_partial(A, h, row0 == 0 ? NaN : 0.f)``).

Two choices on the reference side that need their reason:
  * nb = 1 (section 4): the bias is one constant per head, which the softmax removes, so ``out`` and g_qkv do not
    depend on the table and "one table row zeroed" leaves the float64 reference where it was; their tooth is one key
    removed from the graph that holds the largest message instead (the plain operator's tooth);
  * section 5 counts the rows whose maximum lies in the first chunk while the last chunk's largest score lies far
    below it.  "Far" is 88 (beyond float32 exp's normal range) where the planted fall reaches it.  The planted part
    of a falling row's score is amp^2 dh^-1/2 (-linspace(-1, 1, n))_j; between key 0 and the last chunk's first key
    3T - C of the 3T graph it falls by amp^2 dh^-1/2 (2 - 2 C / (3T - 1)): 116 at (2, 8), amp = 14, but 67.8 at
    (3, 4), amp = 9 and 83.8 at (1, 64), amp = 20.  The threshold is therefore min(88, 0.75 * 2 amp^2 dh^-1/2) =
    88, 60.75 and 75: with the amplitudes fixed, 88 is out of reach at two of the three shapes.

The largest case has 655 rows (section 3: 11 graphs of 2, T + 1, 2T + 1 nodes in turn)."""
import pytest
import torch

import tests.test_gpu_attention as TA
import tests.test_gpu_attention_bias as TB
from graph_hscn import _hip
from graph_hscn.nn import functional as Fh
from tests import attention_bias_oracle as BO
from tests import attention_oracle as AO
from tests.helpers import DEV, TermMagnitudes, check_f64, f64_close, referee_all, teeth

pytestmark = pytest.mark.gpu

NAN_FILL, ZERO_FILL = float("nan"), 0.0


def _tc():
    return int(_hip.lib().hscn_attention_tile()), int(_hip.lib().hscn_attention_chunk())


def _flag():
    return int(Fh.attention_flags(DEV).item())


def _ranges(ptr):
    p = [int(v) for v in ptr]
    return [(p[g], p[g + 1]) for g in range(len(p) - 1)]


def _plant(qkv, ptr, heads, dh, amp):
    """Section 5's direction: column 0 of every head's Q slice := amp (+1, -1, 0)[i % 3] (i the row inside its graph),
    of its K slice := amp linspace(-1, 1, n)."""
    D = heads * dh
    sign = torch.tensor([1.0, -1.0, 0.0])
    for s, e in _ranges(ptr):
        if e > s:
            for h in range(heads):
                qkv[s:e, h * dh] = amp * sign[torch.arange(e - s) % 3]
                qkv[s:e, D + h * dh] = amp * torch.linspace(-1.0, 1.0, e - s)
    return qkv


# --------------------------------------------------------------------------- #
# the plain operator: one case = inputs and CPU references, computed once and shared (never modified)
# --------------------------------------------------------------------------- #
_PLAIN = {}


def _plain_case(key, sizes, heads, dh, seed, amp=None):
    if key not in _PLAIN:
        ptr = TA._ptr(sizes)
        g = torch.Generator().manual_seed(seed)
        N, D = int(ptr[-1]), heads * dh
        qkv = torch.randn(N, 3 * D, generator=g)
        g_out = torch.randn(N, D, generator=g)
        if amp is not None:
            _plant(qkv, ptr, heads, dh, amp)
        out64, lse64 = AO.forward(qkv.double(), ptr, heads)
        a, mag, n = AO.magnitudes(qkv, ptr, heads)
        where = AO.largest_message(qkv, ptr, heads)
        _PLAIN[key] = dict(
            sizes=sizes, ptr=ptr, qkv=qkv, g_out=g_out, out64=out64, lse64=lse64, a=a, mag=mag, n=n,
            n_out=n + 4 + 2 * (dh + 2) * a.repeat_interleave(dh, 1),
            dropped=AO.drop_message(out64, qkv, ptr, heads, where),
            g32=AO.autograd_backward(qkv, ptr, heads, g_out, torch.float32)[1],
            g64=AO.autograd_backward(qkv, ptr, heads, g_out, torch.float64)[1],
            d64=AO.autograd_backward(qkv, ptr, heads, g_out, torch.float64, skip=(where[0], where[1]))[1])
    return _PLAIN[key]


def _plain_lse(qkv, ptr, heads, max_nodes):
    """tests/test_gpu_attention.py's ``_lse_of`` with ``max_nodes`` as given: (out, lse) of the raw entry point."""
    q = qkv.to(DEV).contiguous()
    N, D = q.size(0), q.size(1) // 3
    ptr32 = ptr.to(torch.int32).to(DEV)
    out, lse = torch.empty(N, D, device=DEV), torch.empty(N, heads, device=DEV)
    _hip.call("hscn_attention_fwd", _hip.ptr(q), _hip.ptr(ptr32), N, ptr32.numel() - 1, int(max_nodes), heads,
              D // heads, _hip.ptr(out), _hip.ptr(lse), _hip.ptr(Fh.attention_flags(DEV)), _hip.stream())
    return out, lse


def _plain_run(qkv, g_out, ptr, heads, max_nodes):
    """{"out", "lse", "g_qkv"} of the plain operator on the device."""
    out, leaf = TA._hip_attention(qkv, ptr, heads, max_nodes=max_nodes, requires_grad=True)
    out.backward(g_out.to(DEV))
    out_raw, lse = _plain_lse(qkv, ptr, heads, max_nodes)
    assert torch.equal(out_raw, out)
    return {"out": out.detach(), "lse": lse, "g_qkv": leaf.grad}


def _check_plain(c, got, heads, dh, what):
    """Section 1's bars of the plain operator."""
    D = heads * dh
    assert got["out"].shape == (c["qkv"].size(0), D)
    check_f64(got["out"], c["out64"], c["mag"], c["n_out"], c["dropped"], what=what + " forward")
    assert f64_close(got["lse"], c["lse64"], c["a"] + 1.0 + c["lse64"].abs(), c["n"] + dh + 6, what=what + " lse")
    g, o32, o64 = TA._thirds(got["g_qkv"], D), TA._thirds(c["g32"], D), TA._thirds(c["g64"], D)
    referee_all(g, o32, o64, what + " backward")
    teeth(g, o32, o64, TA._thirds(c["d64"], D), what + " backward [one key removed]")
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# the biased operator
# --------------------------------------------------------------------------- #
_BIAS = {}


def _run_without_key(c, heads, skip):
    """``BO.run`` in float64 with key ``skip = (g, j)`` left out (tests/attention_oracle.py's toothed variant)."""
    x = c["qkv"].double().requires_grad_(True)
    t = c["table"].double().requires_grad_(True)
    out, _ = BO.forward(x, t, c["buckets"], c["ptr"], heads, skip=skip)
    out.backward(c["g_out"].double())
    D = x.size(1) // 3
    return {"out": out.detach(), "gQ": x.grad[:, :D], "gK": x.grad[:, D:2 * D], "gV": x.grad[:, 2 * D:]}


def _bias_case(key, sizes, heads, dh, nb, seed, raw=None, amp=None, table_scale=1.0):
    """``raw``: callable(generator) -> the list of uint8 matrices the device gets (default: uniform below nb); the
    oracle gets them clamped to nb - 1."""
    if key not in _BIAS:
        ptr = TA._ptr(sizes)
        g = torch.Generator().manual_seed(seed)
        N, D = int(ptr[-1]), heads * dh
        qkv = torch.randn(N, 3 * D, generator=g)
        g_out = torch.randn(N, D, generator=g)
        table = torch.randn(nb, heads, generator=g) * table_scale
        if amp is not None:
            _plant(qkv, ptr, heads, dh, amp)
        if raw is None:
            raw = [torch.randint(0, nb, (n, n), dtype=torch.uint8, generator=g) for n in sizes]
        else:
            raw = raw(g)
        buckets = [m.clamp(max=nb - 1) for m in raw]
        c = dict(sizes=sizes, ptr=ptr, qkv=qkv, g_out=g_out, table=table, nb=nb, raw=raw, buckets=buckets,
                 o32=BO.run(qkv, table, buckets, ptr, heads, g_out, torch.float32),
                 o64=BO.run(qkv, table, buckets, ptr, heads, g_out, torch.float64))
        mag, count, gt, (val, b, h) = BO.table_terms(qkv, table, buckets, ptr, heads, g_out)
        assert float((gt - c["o64"]["g_table"]).abs().max()) <= 1e-11 * float(mag.max())    # the formula is autograd's
        assert int(count.sum()) == sum(n * n for n in sizes)
        dropped = c["o64"]["g_table"].clone()
        dropped[b, h] -= val
        c.update(mag_t=mag, dropped_table=dropped)
        if nb > 1:                                          # the row that carries the most bias over its pairs, zeroed
            zeroed = table.clone()
            zeroed[int((count.double() * table.abs().sum(1).double()).argmax())] = 0.0
            z64 = BO.run(qkv, zeroed, buckets, ptr, heads, g_out, torch.float64)
            c.update(tooth={k: z64[k] for k in ("out", "gQ", "gK", "gV")}, tooth_name="one table row zeroed")
        else:                                               # one bucket: the table does not reach out or g_qkv
            where = AO.largest_message(qkv, ptr, heads)
            c.update(tooth=_run_without_key(c, heads, (where[0], where[1])), tooth_name="one key removed")
        _BIAS[key] = c
    return _BIAS[key]


def _terms(c, dh, max_nodes):
    """tests/test_gpu_attention_bias.py's ``_table_terms`` for the case's own B, n_max and the ``max_nodes`` passed."""
    terms = TermMagnitudes(torch.nn.Module(), chain_extra=(dh + 2) + (max(c["sizes"]) + 4) + dh + dh)
    terms._add("g_table", c["mag_t"], TB._sum_depth(len(c["sizes"]), max_nodes))
    return terms


def _spd(c, max_nodes, raw=None):
    data, sptr = BO.flat(c["raw"] if raw is None else raw)
    return Fh.SPDBuckets(data.to(DEV), sptr.to(DEV), c["nb"] - 1, max_nodes)


def _bias_run(c, heads, max_nodes, ptr=None, qkv=None, g_out=None, raw=None):
    """{"out", "gQ", "gK", "gV", "g_table"} of the biased operator on the device (``_hip_run`` with the case's bucket
    count and the ``max_nodes`` given)."""
    ptr = c["ptr"] if ptr is None else ptr
    q = (c["qkv"] if qkv is None else qkv).to(DEV).requires_grad_(True)
    t = c["table"].to(DEV).requires_grad_(True)
    out = Fh.BiasedSelfAttentionFn.apply(q, t, _spd(c, max_nodes, raw), ptr.to(torch.int32).to(DEV), max_nodes, heads)
    out.backward((c["g_out"] if g_out is None else g_out).to(DEV))
    D = q.size(1) // 3
    return {"out": out.detach(), "gQ": q.grad[:, :D], "gK": q.grad[:, D:2 * D], "gV": q.grad[:, 2 * D:],
            "g_table": t.grad}


def _bias_lse(c, heads, max_nodes, ptr=None, qkv=None, raw=None):
    """(out, lse) of the raw biased forward."""
    q = (c["qkv"] if qkv is None else qkv).to(DEV).contiguous()
    N, D = q.size(0), q.size(1) // 3
    ptr32 = (c["ptr"] if ptr is None else ptr).to(torch.int32).to(DEV)
    spd, t = _spd(c, max_nodes, raw), c["table"].to(DEV)
    out, lse = torch.empty(N, D, device=DEV), torch.empty(N, heads, device=DEV)
    _hip.call("hscn_attention_bias_fwd", _hip.ptr(q), _hip.ptr(t), _hip.ptr(spd.bucket), _hip.ptr(spd.spd_ptr),
              _hip.ptr(ptr32), N, ptr32.numel() - 1, spd.bucket.numel(), int(max_nodes), heads, D // heads, c["nb"],
              _hip.ptr(out), _hip.ptr(lse), _hip.ptr(Fh.attention_flags(DEV)), _hip.stream())
    torch.cuda.synchronize()
    return out, lse


def _check_bias(c, got, heads, dh, max_nodes, what):
    """Section 1's bars of the biased operator."""
    assert got["out"].shape == (c["qkv"].size(0), heads * dh) and got["g_table"].shape == (c["nb"], heads)
    terms = _terms(c, dh, max_nodes)
    # g_table: every row's ds_ij add up to zero, so a bucket's sum cancels (with nb = 1 to exactly zero) and the
    # referee's scale max|g_table| says little about its float32 residue (tests/test_gpu_attention_bias.py's header)
    referee_all(got, c["o32"], c["o64"], what, terms=terms, cancelling=["g_table"])
    teeth(got, c["o32"], c["o64"], c["tooth"], f"{what} [{c['tooth_name']}]")
    terms.bound_teeth(got, c["o32"], c["o64"], [dict(c["o64"], g_table=c["dropped_table"])], ["g_table"], what)
    assert _flag() == 0
    return terms


# --------------------------------------------------------------------------- #
# 1. every width of the dispatch ladder
# --------------------------------------------------------------------------- #
WIDTHS = list(range(4, 65, 4))


def _ladder_sizes():
    T, C = _tc()
    return [C + 1, 1, 0, T + 1, 2]


def test_the_envelope_answers_for_every_width_and_refuses_beside_it():
    L = _hip.lib()
    assert len(WIDTHS) == 16
    for dh in WIDTHS:
        assert L.hscn_attention_supported(2, dh) == 1, dh
    for dh in (0, 2, 6, 68):
        assert L.hscn_attention_supported(2, dh) == 0, dh
    assert L.hscn_attention_supported(9, 64) == 0             # D = 576 > 512
    assert L.hscn_attention_supported(8, 64) == 1


@pytest.mark.parametrize("dh", WIDTHS)
def test_plain_attention_at_every_head_width(dh):
    heads, sizes = 2, _ladder_sizes()
    assert sum(sizes) == 101
    c = _plain_case(("ladder", dh), sizes, heads, dh, seed=1000 + dh)
    got = _plain_run(c["qkv"], c["g_out"], c["ptr"], heads, max(sizes))
    _check_plain(c, got, heads, dh, f"plain attention dh={dh}")


@pytest.mark.parametrize("dh", WIDTHS)
def test_biased_attention_at_every_head_width(dh):
    heads, sizes = 2, _ladder_sizes()
    c = _bias_case(("ladder", dh), sizes, heads, dh, nb=5, seed=2000 + dh)
    got = _bias_run(c, heads, max(sizes))
    _check_bias(c, got, heads, dh, max(sizes), f"biased attention dh={dh}")


# --------------------------------------------------------------------------- #
# 2. more than two tiles, idle tiles, many chunks
# --------------------------------------------------------------------------- #
TILE_SHAPES = [(1, 4), (3, 8), (2, 64)]


def _tile_sizes():
    T, C = _tc()
    return [2 * T + 1, 1, 3 * T, 0, C - 1]


@pytest.mark.parametrize("heads,dh", TILE_SHAPES)
def test_plain_attention_over_three_tiles_with_and_without_idle_tiles(heads, dh):
    T, C = _tc()
    sizes = _tile_sizes()
    c = _plain_case(("tiles", heads, dh), sizes, heads, dh, seed=3000 + 100 * heads + dh)
    qkv, g_out, ptr = c["qkv"], c["g_out"], c["ptr"]
    tight = _plain_run(qkv, g_out, ptr, heads, 3 * T)
    idle = _plain_run(qkv, g_out, ptr, heads, 5 * T + 1)      # six tiles per graph, three or more of them without rows
    _check_plain(c, tight, heads, dh, f"plain attention heads={heads} dh={dh} max_nodes=3T")
    _check_plain(c, idle, heads, dh, f"plain attention heads={heads} dh={dh} max_nodes=5T+1")
    for k in ("out", "lse", "g_qkv"):
        assert torch.equal(tight[k], idle[k]), k
    # a graph alone has the bits it has inside the batch: the last one (as the neighbouring files test it) and the
    # two whose rows reach the third tile, row0 = 2 * AT_TILE
    for g in (4, 2, 0):
        s, e = int(ptr[g]), int(ptr[g + 1])
        alone = _plain_run(qkv[s:e], g_out[s:e], TA._ptr([e - s]), heads, e - s)
        for k in ("out", "lse", "g_qkv"):
            assert torch.equal(tight[k][s:e], alone[k]), (k, g)
    assert _flag() == 0


@pytest.mark.parametrize("heads,dh", TILE_SHAPES)
def test_biased_attention_over_three_tiles_with_and_without_idle_tiles(heads, dh):
    T, C = _tc()
    sizes = _tile_sizes()
    c = _bias_case(("tiles", heads, dh), sizes, heads, dh, nb=6, seed=4000 + 100 * heads + dh)
    ptr = c["ptr"]
    tight, idle = _bias_run(c, heads, 3 * T), _bias_run(c, heads, 5 * T + 1)
    _check_bias(c, tight, heads, dh, 3 * T, f"biased attention heads={heads} dh={dh} max_nodes=3T")
    _check_bias(c, idle, heads, dh, 5 * T + 1, f"biased attention heads={heads} dh={dh} max_nodes=5T+1")
    # g_table too: the second run's fold adds 15 further partials, all of them +0.0 from tiles without rows, and
    # x + (+0.0) = x for every float x that a sum can hold here (a sum that starts at +0.0 is never -0.0)
    for k in ("out", "gQ", "gK", "gV", "g_table"):
        assert torch.equal(tight[k], idle[k]), k
    (out_t, lse_t), (out_i, lse_i) = _bias_lse(c, heads, 3 * T), _bias_lse(c, heads, 5 * T + 1)
    assert torch.equal(lse_t, lse_i) and torch.equal(out_t, tight["out"]) and torch.equal(out_i, tight["out"])
    for g in (4, 2, 0):
        s, e = int(ptr[g]), int(ptr[g + 1])
        one = dict(ptr=TA._ptr([e - s]), qkv=c["qkv"][s:e], raw=c["raw"][g:g + 1])
        alone = _bias_run(c, heads, e - s, g_out=c["g_out"][s:e], **one)
        for k in ("out", "gQ", "gK", "gV"):
            assert torch.equal(tight[k][s:e], alone[k]), (k, g)
        assert torch.equal(lse_t[s:e], _bias_lse(c, heads, e - s, **one)[1]), ("lse", g)
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# 3. the fold at its block edges
# --------------------------------------------------------------------------- #
FOLD_TABLES = [(1, 64), (4, 17), (2, 33)]                     # heads * nb = 64, 68, 66
FOLD_LAUNCHES = ["31", "32", "33", "65", "11x3"]              # tiles in the launch: B x 1, and 11 graphs x 3 tiles


def _fold_batch(launch):
    """(sizes, max_nodes, tiles in the launch)"""
    T, _ = _tc()
    if launch == "11x3":
        sizes, mn = [(2, T + 1, 2 * T + 1)[g % 3] for g in range(11)], 2 * T + 1
    else:
        sizes, mn = [(2, 3, 4, 5)[g % 4] for g in range(int(launch))], 5
    return sizes, mn, len(sizes) * max(1, -(-mn // T))


def _raw_bias_backward(c, heads, dh, max_nodes, fwd_max_nodes=None, bucket=None, fill=NAN_FILL):
    """The biased backward pair through the raw entry points with a workspace of the caller's: (g_qkv, delta, g_table,
    workspace [tiles, heads, nb]).  ``out`` and ``lse`` come from a forward with ``fwd_max_nodes`` and the case's whole
    bucket tensor; ``bucket`` replaces the bucket tensor of the backward pair.  ``fill``: what the workspace and g_table
    hold before the launch (NaN: a partial or an entry that is not written shows)."""
    T, _ = _tc()
    q, go, t = c["qkv"].to(DEV).contiguous(), c["g_out"].to(DEV).contiguous(), c["table"].to(DEV)
    N, D, B, nb = q.size(0), q.size(1) // 3, len(c["sizes"]), c["nb"]
    ptr32 = c["ptr"].to(torch.int32).to(DEV)
    fmn = max_nodes if fwd_max_nodes is None else fwd_max_nodes
    spd = _spd(c, fmn)
    flag = _hip.ptr(Fh.attention_flags(DEV))
    out, lse = torch.empty(N, D, device=DEV), torch.empty(N, heads, device=DEV)
    _hip.call("hscn_attention_bias_fwd", _hip.ptr(q), _hip.ptr(t), _hip.ptr(spd.bucket), _hip.ptr(spd.spd_ptr),
              _hip.ptr(ptr32), N, B, spd.bucket.numel(), int(fmn), heads, dh, nb, _hip.ptr(out), _hip.ptr(lse), flag,
              _hip.stream())
    bk = spd.bucket if bucket is None else bucket
    tiles = B * max(1, -(-max_nodes // T))
    work = torch.full((tiles * heads * nb,), fill, device=DEV)
    g_qkv, delta = torch.zeros(N, 3 * D, device=DEV), torch.zeros(N, heads, device=DEV)
    g_table = torch.full((nb, heads), fill, device=DEV)
    _hip.call("hscn_attention_bias_bwd_q", _hip.ptr(q), _hip.ptr(out), _hip.ptr(lse), _hip.ptr(go), _hip.ptr(t),
              _hip.ptr(bk), _hip.ptr(spd.spd_ptr), _hip.ptr(ptr32), N, B, bk.numel(), int(max_nodes), heads, dh, nb,
              _hip.ptr(g_qkv), _hip.ptr(delta), _hip.ptr(g_table), _hip.ptr(work), work.numel(), flag, _hip.stream())
    _hip.call("hscn_attention_bias_bwd_kv", _hip.ptr(q), _hip.ptr(lse), _hip.ptr(delta), _hip.ptr(go), _hip.ptr(t),
              _hip.ptr(bk), _hip.ptr(spd.spd_ptr), _hip.ptr(ptr32), N, B, bk.numel(), int(max_nodes), heads, dh, nb,
              _hip.ptr(g_qkv), flag, _hip.stream())
    torch.cuda.synchronize()
    return g_qkv, delta, g_table, work.view(tiles, heads, nb)


@pytest.mark.parametrize("heads,nb", FOLD_TABLES)
@pytest.mark.parametrize("launch", FOLD_LAUNCHES)
def test_the_fold_adds_every_partial_once_in_tile_order(launch, heads, nb):
    T, _ = _tc()
    dh = 4
    sizes, mn, tiles = _fold_batch(launch)
    assert tiles == {"31": 31, "32": 32, "33": 33, "65": 65, "11x3": 33}[launch]
    c = _bias_case(("fold", launch, heads, nb), sizes, heads, dh, nb, seed=5000 + 100 * heads + nb + len(sizes))
    what = f"fold tiles={launch} heads={heads} nb={nb}"
    got = _bias_run(c, heads, mn)
    _check_bias(c, got, heads, dh, mn, what)
    again = _bias_run(c, heads, mn)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    # the fold alone: g_table is the float32 sum of the partials in tile order, [tile, head, bucket] -> [bucket, head]
    g_qkv, _, g_table, part = _raw_bias_backward(c, heads, dh, mn)
    part = part.cpu()
    assert part.shape == (tiles, heads, nb) and not bool(torch.isnan(part).any())
    acc = torch.zeros(heads, nb, dtype=torch.float32)
    for t in range(tiles):
        acc = acc + part[t]
    assert torch.equal(g_table.cpu(), acc.t().contiguous())
    assert torch.equal(g_table, got["g_table"])
    assert torch.equal(g_qkv, torch.cat([got["gQ"], got["gK"], got["gV"]], 1))
    if launch == "11x3":                                      # tiles without rows wrote zeros, tiles with rows did not
        per = mn // T + 1
        for g, n in enumerate(sizes):
            for t in range(per):
                zero = bool((part[g * per + t] == 0).all())
                assert zero == (t * T >= n), (g, t)
    assert _flag() == 0


# --------------------------------------------------------------------------- #
# 4. bucket count and bucket bytes
# --------------------------------------------------------------------------- #
BUCKET_SHAPES = [(4, 8), (2, 64)]
CLAMP_BYTES = [0, 1, 2, 3, 4, 5, 6, 7, 200, 255]


def _bucket_sizes():
    T, C = _tc()
    return [1, C + 1, T + 1, 0, 5]


@pytest.mark.parametrize("heads,dh", BUCKET_SHAPES)
@pytest.mark.parametrize("nb", [1, 2, 63, 64])
def test_biased_attention_at_the_ends_of_the_bucket_count(nb, heads, dh):
    sizes = _bucket_sizes()
    c = _bias_case(("count", heads, dh, nb), sizes, heads, dh, nb, seed=6000 + 1000 * heads + 10 * dh + nb)
    assert max(int(m.max()) for m in c["raw"] if m.numel()) == nb - 1
    got = _bias_run(c, heads, max(sizes))
    terms = _check_bias(c, got, heads, dh, max(sizes), f"biased attention heads={heads} dh={dh} nb={nb}")
    if nb == 1:
        # g_table[0, h] = the sum of ALL ds_ij: zero in exact arithmetic, float32 residue on the device.  The referee's
        # scale means nothing here; the a-priori bound is the bar
        assert float(c["o64"]["g_table"].abs().max()) <= 1e-12 * float(c["mag_t"].max())
        assert terms.bound_holds("g_table", got["g_table"], c["o64"]["g_table"], "nb=1")


@pytest.mark.parametrize("heads,dh", BUCKET_SHAPES)
def test_a_bucket_byte_beyond_the_table_is_read_as_the_last_bucket(heads, dh):
    sizes, nb = _bucket_sizes(), 6
    values = torch.tensor(CLAMP_BYTES, dtype=torch.uint8)

    def raw(g):
        return [values[torch.randint(0, len(CLAMP_BYTES), (n, n), generator=g)] for n in sizes]

    c = _bias_case(("clamp", heads, dh), sizes, heads, dh, nb, seed=7000 + 100 * heads + dh, raw=raw)
    assert sum(n > 10 for n in sizes) == 2
    for n, m in zip(sizes, c["raw"]):
        if n > 10:
            assert sorted(set(m.reshape(-1).tolist())) == CLAMP_BYTES
    what = f"biased attention heads={heads} dh={dh} nb=6 with bytes up to 255"
    got = _bias_run(c, heads, max(sizes))                     # the device reads the raw bytes
    terms = _check_bias(c, got, heads, dh, max(sizes), what)
    # the bytes >= nb read as bucket 0 instead of nb - 1: gK is there because k_attn_bwd_kv clamps on its own
    as_zero = [torch.where(m >= nb, torch.zeros_like(m), m) for m in c["raw"]]
    w64 = BO.run(c["qkv"], c["table"], as_zero, c["ptr"], heads, c["g_out"], torch.float64)
    teeth(got, c["o32"], c["o64"], {k: w64[k] for k in ("out", "gK", "g_table")}, what + " [read as bucket 0]")
    assert not terms.bound_holds("g_table", got["g_table"], w64["g_table"], what + " [read as bucket 0]")


# --------------------------------------------------------------------------- #
# 5. the running maximum
# --------------------------------------------------------------------------- #
SOFTMAX_SHAPES = [(2, 8, 14.0), (3, 4, 9.0), (1, 64, 20.0)]


def _softmax_sizes():
    T, C = _tc()
    return [1, 2 * T + 1, C + 1, 0, 3 * T, 5]


def _assert_rows_rise_and_fall(c, heads, dh, amp, table=None):
    """From the float64 scores of the 3T graph: at least 32 (row, head) pairs have their maximum in the last chunk, and
    at least 32 have it in the first chunk with the last chunk's largest score far below (this file's header)."""
    T, C = _tc()
    g = 4
    s, e = int(c["ptr"][g]), int(c["ptr"][g + 1])
    assert e - s == 3 * T
    far = min(88.0, 0.75 * 2.0 * amp * amp * dh ** -0.5)
    D = heads * dh
    qkv = c["qkv"].double()
    rising = falling = 0
    for h in range(heads):
        S = qkv[s:e, h * dh:(h + 1) * dh] @ qkv[s:e, D + h * dh:D + (h + 1) * dh].t() * dh ** -0.5
        if table is not None:
            S = S + table.double()[c["buckets"][g].long()][:, :, h]
        at = S.argmax(1)
        rising += int((at >= e - s - C).sum())
        falling += int(((at < C) & (S.max(1).values - S[:, e - s - C:].max(1).values > far)).sum())
    assert rising >= 32 and falling >= 32, (rising, falling, far)


@pytest.mark.parametrize("heads,dh,amp", SOFTMAX_SHAPES)
def test_plain_attention_keeps_a_running_maximum(heads, dh, amp):
    sizes = _softmax_sizes()
    c = _plain_case(("softmax", heads, dh), sizes, heads, dh, seed=8000 + 100 * heads + dh, amp=amp)
    _assert_rows_rise_and_fall(c, heads, dh, amp)
    got = _plain_run(c["qkv"], c["g_out"], c["ptr"], heads, max(sizes))
    assert bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["g_qkv"]).all())
    assert bool(torch.isfinite(got["lse"]).all())
    _check_plain(c, got, heads, dh, f"plain attention heads={heads} dh={dh} logits of +-{amp * amp * dh ** -0.5:.0f}")


@pytest.mark.parametrize("heads,dh,amp", SOFTMAX_SHAPES)
def test_biased_attention_keeps_a_running_maximum(heads, dh, amp):
    sizes = _softmax_sizes()
    c = _bias_case(("softmax", heads, dh), sizes, heads, dh, nb=6, seed=9000 + 100 * heads + dh, amp=amp,
                   table_scale=3.0)
    _assert_rows_rise_and_fall(c, heads, dh, amp, table=c["table"])
    got = _bias_run(c, heads, max(sizes))
    for k in ("out", "gQ", "gK", "gV", "g_table"):
        assert bool(torch.isfinite(got[k]).all()), k
    _check_bias(c, got, heads, dh, max(sizes),
                f"biased attention heads={heads} dh={dh} logits of +-{amp * amp * dh ** -0.5:.0f}")


# --------------------------------------------------------------------------- #
# 6. refusals seen from the backward
# --------------------------------------------------------------------------- #
REFUSAL_HEADS, REFUSAL_DH = 4, 8


def _refusal_sizes():
    T, _ = _tc()
    return [5, T + 1, 3]


def _raw_plain_backward(c, heads, dh, max_nodes, fwd_max_nodes):
    q, go = c["qkv"].to(DEV).contiguous(), c["g_out"].to(DEV).contiguous()
    N, D, B = q.size(0), q.size(1) // 3, len(c["sizes"])
    ptr32 = c["ptr"].to(torch.int32).to(DEV)
    flag = _hip.ptr(Fh.attention_flags(DEV))
    out, lse = _plain_lse(c["qkv"], c["ptr"], heads, fwd_max_nodes)
    g_qkv, delta = torch.zeros(N, 3 * D, device=DEV), torch.zeros(N, heads, device=DEV)
    _hip.call("hscn_attention_bwd_q", _hip.ptr(q), _hip.ptr(out), _hip.ptr(lse), _hip.ptr(go), _hip.ptr(ptr32), N, B,
              int(max_nodes), heads, dh, _hip.ptr(g_qkv), _hip.ptr(delta), flag, _hip.stream())
    _hip.call("hscn_attention_bwd_kv", _hip.ptr(q), _hip.ptr(lse), _hip.ptr(delta), _hip.ptr(go), _hip.ptr(ptr32), N, B,
              int(max_nodes), heads, dh, _hip.ptr(g_qkv), flag, _hip.stream())
    torch.cuda.synchronize()
    return g_qkv, delta


def _assert_refused_rows(c, bad, good, refused, D):
    """``bad`` / ``good`` = (g_qkv, delta) of the refusing and the truthful run: NaN in the refused graphs' rows of all
    three thirds and of delta, the truthful run's bits everywhere else."""
    rows = torch.zeros(c["qkv"].size(0), dtype=torch.bool)
    for g in refused:
        rows[int(c["ptr"][g]):int(c["ptr"][g + 1])] = True
    assert 0 < int(rows.sum()) < rows.numel()
    rows = rows.to(DEV)
    for name, b, a in (("gQ", bad[0][:, :D], good[0][:, :D]), ("gK", bad[0][:, D:2 * D], good[0][:, D:2 * D]),
                       ("gV", bad[0][:, 2 * D:], good[0][:, 2 * D:]), ("delta", bad[1], good[1])):
        assert bool(torch.isnan(b[rows]).all()), name
        assert torch.equal(b[~rows], a[~rows]) and bool(torch.isfinite(a).all()), name


def _assert_flag_raises(bit, match):
    assert _flag() == bit
    with pytest.raises(ValueError, match=match):
        Fh.check_attention(DEV)
    assert _flag() == 0                                       # read and cleared


def test_the_plain_backward_refuses_a_graph_beyond_max_nodes():
    T, _ = _tc()
    heads, dh, sizes = REFUSAL_HEADS, REFUSAL_DH, _refusal_sizes()
    c = _plain_case(("refusal",), sizes, heads, dh, seed=11)
    assert _flag() == 0
    good = _raw_plain_backward(c, heads, dh, T + 1, T + 1)
    assert _flag() == 0
    bad = _raw_plain_backward(c, heads, dh, T, T + 1)         # out and lse of a truthful forward; one tile per graph
    _assert_flag_raises(Fh.ATTN_GRAPH_TOO_LARGE, "max_nodes")
    _assert_refused_rows(c, bad, good, [1], heads * dh)


def test_the_biased_backward_refuses_a_graph_beyond_max_nodes():
    T, _ = _tc()
    heads, dh, sizes = REFUSAL_HEADS, REFUSAL_DH, _refusal_sizes()
    c = _bias_case(("refusal",), sizes, heads, dh, nb=6, seed=12)
    assert _flag() == 0
    good = _raw_bias_backward(c, heads, dh, T + 1, T + 1, fill=ZERO_FILL)
    assert _flag() == 0 and bool(torch.isfinite(good[2]).all())
    bad = _raw_bias_backward(c, heads, dh, T, T + 1, fill=ZERO_FILL)
    _assert_flag_raises(Fh.ATTN_GRAPH_TOO_LARGE, "max_nodes")
    _assert_refused_rows(c, bad[:2], good[:2], [1], heads * dh)
    # the refused graph's one tile wrote a NaN partial for every (head, bucket); the fold carries it to every entry
    part = bad[3].cpu()
    assert part.shape == (3, heads, 6) and bool(torch.isnan(part[1]).all())
    assert not bool(torch.isnan(part[0]).any()) and not bool(torch.isnan(part[2]).any())
    assert bool(torch.isnan(bad[2]).all())


def test_the_biased_backward_refuses_buckets_of_another_batch():
    T, _ = _tc()
    heads, dh, sizes = REFUSAL_HEADS, REFUSAL_DH, _refusal_sizes()
    c = _bias_case(("refusal",), sizes, heads, dh, nb=6, seed=12)
    assert _flag() == 0
    good = _raw_bias_backward(c, heads, dh, T + 1, fill=ZERO_FILL)
    assert _flag() == 0
    # the first 100 bytes of the bucket tensor: graph 0's 25 are all there, the ranges of graphs 1 and 2 leave it
    short = BO.flat(c["raw"])[0][:100].to(DEV)
    assert sizes[0] ** 2 <= 100 < sizes[0] ** 2 + sizes[1] ** 2
    bad = _raw_bias_backward(c, heads, dh, T + 1, bucket=short, fill=ZERO_FILL)
    _assert_flag_raises(Fh.ATTN_BUCKETS_OUT_OF_RANGE, "bucket range")
    _assert_refused_rows(c, bad[:2], good[:2], [1, 2], heads * dh)
    part = bad[3].cpu()                                       # two tiles per graph: NaN from a refused graph's first
    assert part.shape == (6, heads, 6)
    assert bool(torch.isnan(part[2]).all()) and bool(torch.isnan(part[4]).all())
    assert bool((part[3] == 0).all()) and bool((part[5] == 0).all()) and bool((part[1] == 0).all())
    assert torch.equal(part[0], good[3].cpu()[0])
    assert bool(torch.isnan(bad[2]).all())
