"""Layered HIP operators against float64 at their dispatch edges.

Every case feeds float32 inputs to one C-ABI entry and compares the result with the same operation evaluated in
float64 on those inputs, under the componentwise a-priori bound of ``helpers.f64_close``.  Every check also proves
its teeth: the same bound must reject a float64 reference with the largest single term removed
(``helpers.check_f64``).  Case ids name the host-code branch they reach (csrc/linear.hip, spmm.hip, gat.hip,
pool.hip, norm.hip, loss.hip).  Where the code claims bit-for-bit agreement -- the CSR walk reproduces the CPU
``index_add_`` order with separately rounded products -- ``torch.equal`` is asserted instead.

The environment-selected variants (``HSCN_LINEAR_BWD_W``, ``HSCN_SPMM_*``, ``HSCN_DENSE_*``) are read once per process by the C side,
so they run this file's cases again in fresh child processes, one at a time."""
import copy
import math
import os
import subprocess
import sys

import pytest
import torch

from graph_hscn import _hip
from graph_hscn._hip import ACT, call, ptr, stream
from tests.helpers import DEV, check_f64, drop_largest_product, f64_close

pytestmark = pytest.mark.gpu

E_UNSUPPORTED_MSG = "failed with code"
ACTS = ["identity", "relu", "elu", "tanh"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _act64(t, act):
    if act == "relu":
        return t.clamp_min(0)
    if act == "elu":
        return torch.where(t > 0, t, torch.expm1(t))
    if act == "tanh":
        return torch.tanh(t)
    return t


def _dev(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


# --------------------------------------------------------------------------- #
# hscn_linear_fwd
# --------------------------------------------------------------------------- #
# id: (rows, I, O, bias, x2, w_layout, act, att)
LINEAR_FWD = {
    "vec4": (300, 16, 16, True, False, 0, "identity", False),
    "vec1_o10": (300, 16, 10, True, False, 0, "identity", False),
    "i_mod4_scalar_loads": (300, 9, 16, True, False, 0, "relu", False),
    "lpr_pow2_o64": (257, 32, 64, True, False, 0, "identity", False),
    "lpr_nonpow2_o48": (257, 32, 48, True, False, 0, "identity", False),
    "rows0": (0, 16, 16, True, False, 0, "identity", False),
    "rows1": (1, 9, 16, True, False, 0, "identity", False),
    "gridstride_past_nb_cap": (140000, 16, 16, True, False, 0, "identity", False),   # RPB 64: 2048 * 64 < rows
    "lds_over_64k_x2": (700, 128, 128, True, True, 0, "identity", False),            # 128 KiB of W + W2 in LDS
    "x2": (300, 12, 16, False, True, 0, "identity", False),
    "no_bias": (300, 16, 16, False, False, 0, "identity", False),
    "w_layout1": (300, 16, 12, False, False, 1, "identity", False),
    "act_relu": (300, 16, 16, True, False, 0, "relu", False),
    "act_elu": (300, 16, 16, True, False, 0, "elu", False),
    "act_tanh": (300, 16, 16, True, False, 0, "tanh", False),
    "att_fused_lpr4": (500, 16, 16, False, False, 0, "identity", True),
    "att_fused_lpr64": (500, 16, 256, False, False, 0, "identity", True),
    "att_rowdot_o12": (500, 16, 12, False, False, 0, "identity", True),                 # LPR 3: k_rowdot
}


@pytest.mark.parametrize("case", list(LINEAR_FWD), ids=list(LINEAR_FWD))
def test_linear_fwd(case):
    rows, I, O, has_b, has_x2, layout, act, has_att = LINEAR_FWD[case]
    g = _gen(len(case) * 7 + rows)
    x = torch.randn(rows, I, generator=g)
    W = torch.randn(O, I, generator=g) / I ** 0.5
    b = torch.randn(O, generator=g) if has_b else None
    x2 = torch.randn(rows, I, generator=g) if has_x2 else None
    W2 = torch.randn(O, I, generator=g) / I ** 0.5 if has_x2 else None
    att = torch.randn(O, generator=g) if has_att else None
    Wc = W.t().contiguous() if layout else W
    W2c = (W2.t().contiguous() if layout else W2) if has_x2 else None
    xd, Wd, bd, x2d, W2d, attd = _dev(x, Wc, b, x2, W2c, att)
    y = torch.empty(rows, O, device=DEV)
    a = torch.empty(max(rows, 1), device=DEV) if has_att else None
    call("hscn_linear_fwd", ptr(xd), ptr(Wd), ptr(bd), ptr(x2d), ptr(W2d), ptr(attd), ptr(a), ptr(y), rows, I, O,
         layout, ACT[act], stream())
    if rows == 0:
        return
    Wt = W.double().t()
    pre = x.double() @ Wt
    mag = x.double().abs() @ Wt.abs()
    n = I + 2
    if has_x2:
        pre = pre + x2.double() @ W2.double().t()
        mag = mag + x2.double().abs() @ W2.double().t().abs()
        n += I
    raw = pre.clone()
    if has_b:
        pre = pre + b.double()
        mag = mag + b.double().abs()
    ref = _act64(pre, act)
    if act != "identity":
        mag = mag + ref.abs()
        n += 4
    dropped = drop_largest_product(ref, x, Wt, post=lambda r, o, t: float(_act64(pre[r, o] - t, act)))
    check_f64(y, ref, mag, n, dropped, what=f"linear {case} y")
    if has_att:
        a64 = raw @ att.double()
        amag = mag @ att.double().abs()
        da = drop_largest_product(a64.view(-1, 1), raw, att.double().view(-1, 1))
        check_f64(a[:rows], a64, amag, I + O + 2, da.view(-1), what=f"linear {case} att")


def test_linear_fwd_refusals():
    x = torch.randn(8, 256, device=DEV)
    W = torch.randn(256, 256, device=DEV)
    y = torch.empty(8, 256, device=DEV)
    with pytest.raises(RuntimeError, match=E_UNSUPPORTED_MSG):   # 256 KiB of W: past the 160 KiB LDS
        call("hscn_linear_fwd", ptr(x), ptr(W), None, None, None, None, None, ptr(y), 8, 256, 256, 0, 0, stream())
    rc = _hip.lib().hscn_linear_fwd(ptr(x), ptr(W), None, None, None, None, None, ptr(y), 8, 256, 256, 0, 0, stream())
    assert rc == _unsupported()
    x = torch.randn(8, 16, device=DEV)
    W = torch.randn(12, 16, device=DEV)
    b = torch.randn(12, device=DEV)
    att = torch.randn(12, device=DEV)
    a = torch.empty(8, device=DEV)
    y = torch.empty(8, 12, device=DEV)
    rc = _hip.lib().hscn_linear_fwd(ptr(x), ptr(W), ptr(b), None, None, ptr(att), ptr(a), ptr(y), 8, 16, 12, 0, 0,
                                    stream())
    assert rc == _unsupported()                                   # att with LPR 3 (k_rowdot) cannot fold the bias


def _unsupported():
    import re
    h = open(os.path.join(os.path.dirname(__file__), "..", "include", "hscn.h")).read()
    return int(re.search(r"HSCN_E_UNSUPPORTED\s*=?\s*\(?(-?\d+)", h).group(1))


# --------------------------------------------------------------------------- #
# hscn_linear_bwd_w
# --------------------------------------------------------------------------- #
# id: (rows, I, O); TO = O / 16, TI = ceil((I + 1) / 16)
BWD_W = {
    "mfma_1x1_i15": (500, 15, 16), "mfma_1x2_i16_bias_col": (500, 16, 16), "mfma_1x3": (500, 40, 16),
    "mfma_1x4": (500, 63, 16), "mfma_2x1": (500, 9, 32), "mfma_2x2": (500, 31, 32), "mfma_2x3": (500, 47, 32),
    "mfma_2x4": (500, 60, 32), "mfma_3x1": (500, 15, 48), "mfma_3x2": (500, 20, 48), "mfma_4x1": (500, 9, 64),
    "mfma_4x2": (500, 16, 64),
    "partial_o10": (500, 9, 10), "partial_tile_product_12": (500, 40, 64),
    "bias_only_i0": (500, 0, 16), "rows_lt_64": (37, 16, 16), "rows_not_chunk_multiple": (1000, 16, 16),
    "rows0": (0, 16, 16), "rows_past_512_chunks": (40000, 16, 32),
}


def _bwd_w(gy, x, I, O, accumulate=0, gW=None, gb=None):
    rows = gy.shape[0]
    gW = torch.empty(O, max(I, 1), device=DEV) if gW is None else gW
    gb = torch.empty(O, device=DEV) if gb is None else gb
    nbytes = int(_hip.lib().hscn_linear_bwd_w_workspace_bytes(rows, I, O))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=DEV)
    call("hscn_linear_bwd_w", ptr(gy), ptr(x) if I else None, ptr(gW) if I else None, ptr(gb), rows, I, O, accumulate,
         ptr(ws), nbytes, stream())
    return gW, gb


def _bwd_w_depth(rows):
    """Longest addition path of the two-stage ordered reduction: a chunk's fma chain, one slice of <= ceil(G / 8)
    chunk partials, the fold of 8 slices, an accumulate."""
    G = min(max((rows + 63) // 64, 1), 512)
    return (rows + G - 1) // G + (G + 7) // 8 + 8 + 2


@pytest.mark.parametrize("case", list(BWD_W), ids=list(BWD_W))
def test_linear_bwd_w(case):
    rows, I, O = BWD_W[case]
    g = _gen(rows + 31 * I + O)
    gy = torch.randn(rows, O, generator=g)
    x = torch.randn(rows, I, generator=g)
    gW, gb = _bwd_w(gy.to(DEV), x.to(DEV) if I else None, I, O)
    n = _bwd_w_depth(rows)
    gy64, x1 = gy.double(), torch.cat([x.double(), torch.ones(rows, 1, dtype=torch.float64)], 1)
    ref = gy64.t() @ x1                                           # [O, I + 1]: the bias is the ones column
    mag = gy64.abs().t() @ x1.abs()
    got = torch.cat([gW.cpu()[:, :I], gb.cpu().view(-1, 1)], 1)
    if rows == 0:
        assert torch.equal(got, torch.zeros(O, I + 1))
        return
    dropped = drop_largest_product(ref, gy64.t(), x1)
    check_f64(got, ref, mag, n, dropped, what=f"bwd_w {case}")


def test_linear_bwd_w_accumulate():
    rows, I, O = 3000, 16, 32
    g = _gen(9)
    gy, x = torch.randn(rows, O, generator=g), torch.randn(rows, I, generator=g)
    W0, b0 = torch.randn(O, I, generator=g), torch.randn(O, generator=g)
    gW, gb = _bwd_w(gy.to(DEV), x.to(DEV), I, O, 1, W0.to(DEV).contiguous(), b0.to(DEV).contiguous())
    x1 = torch.cat([x.double(), torch.ones(rows, 1, dtype=torch.float64)], 1)
    base = torch.cat([W0.double(), b0.double().view(-1, 1)], 1)
    ref = base + gy.double().t() @ x1
    mag = base.abs() + gy.double().abs().t() @ x1.abs()
    got = torch.cat([gW.cpu(), gb.cpu().view(-1, 1)], 1)
    check_f64(got, ref, mag, _bwd_w_depth(rows), drop_largest_product(ref, gy.double().t(), x1), what="bwd_w acc")
    # accumulate = 1 adds to what is there: the base itself is the largest single term it could lose
    assert not f64_close(got, ref - base, mag, _bwd_w_depth(rows))


# --------------------------------------------------------------------------- #
# hscn_act_fwd / hscn_act_bwd
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("act", ["relu", "elu", "tanh"])
def test_act_fwd_bwd(act):
    g = _gen(ACT[act])
    x = torch.cat([torch.randn(5000, generator=g) * 3, torch.tensor([-100.0, -30.0, -1e-6, 0.0, 1e-6, 12.0, 40.0])])
    gy = torch.randn(x.numel(), generator=g)
    xd, gyd = _dev(x, gy)
    y = torch.empty_like(xd)
    call("hscn_act_fwd", ptr(xd), ptr(y), x.numel(), ACT[act], stream())
    ref = _act64(x.double(), act)
    k = int((ref - _act64(torch.zeros_like(ref), act)).abs().argmax())
    dropped = ref.clone()
    dropped[k] = float(_act64(torch.zeros(1, dtype=torch.float64), act))       # the element's one term removed
    check_f64(y, ref, ref.abs() + 2 ** -126, 4, dropped, what=f"act fwd {act}")
    gx = torch.empty_like(xd)
    call("hscn_act_bwd", ptr(gyd), ptr(y), ptr(gx), x.numel(), ACT[act], stream())
    y64 = y.cpu().double()                        # the backward reads y: its derivative is exact from the output
    d = {"relu": (y64 > 0).double(), "elu": torch.where(y64 > 0, torch.ones_like(y64), y64 + 1),
         "tanh": 1 - y64 * y64}[act]
    gref = gy.double() * d
    # the derivative is rounded from y: 1 - y^2 (tanh) and y + 1 (elu) carry an error of u (y^2 + 1), u (|y| + 1)
    dmag = {"relu": d, "elu": y64.abs() + 1, "tanh": y64 * y64 + 1}[act]
    gmag = gy.double().abs() * dmag
    k = int(gref.abs().argmax())
    gdrop = gref.clone()
    gdrop[k] = 0
    check_f64(gx, gref, gmag + 1e-300, 4, gdrop, what=f"act bwd {act}")


def test_act_gridstride_past_block_cap():
    """count > 4096 blocks x 256 threads: every element of the grid-stride tail is written (each act once)."""
    count = 4096 * 256 + 123457
    x = torch.randn(count, generator=_gen(3)).to(DEV)
    for act in ("relu", "elu", "tanh"):
        y = torch.full_like(x, float("nan"))
        call("hscn_act_fwd", ptr(x), ptr(y), count, ACT[act], stream())
        ref = _act64(x.cpu().double(), act)
        # the element of the grid-stride tail that the bound sees best, without its input: act(0)
        tail = 4096 * 256
        k = tail + int((ref[tail:] - _act64(torch.zeros(1, dtype=torch.float64), act)).abs().argmax())
        dropped = ref.clone()
        dropped[k] = float(_act64(torch.zeros(1, dtype=torch.float64), act))
        check_f64(y, ref, ref.abs() + 2 ** -126, 4, dropped, what=f"act tail {act}")
        g = torch.full_like(x, float("nan"))
        call("hscn_act_bwd", ptr(x), ptr(y), ptr(g), count, ACT[act], stream())
        assert bool(torch.isfinite(g).all())


# --------------------------------------------------------------------------- #
# hscn_spmm_csr_gcn / hscn_spmm_csr_weighted
# --------------------------------------------------------------------------- #
def _graph_with_degrees(n, hub, seed, degs=(0, 1, 2, 3, 4, 5, 8)):
    """dst-keyed edge list: row r has degs[r % len(degs)] in-edges, row 1 (when hub) several thousand."""
    g = _gen(seed)
    d = torch.tensor(degs)[torch.arange(n) % len(degs)]
    if hub:
        d[1] = hub
    dst = torch.repeat_interleave(torch.arange(n), d)
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)          # the CSR build sorts stably: any input order
    return torch.stack([src[perm], dst[perm]])


def _rel(ei, n):
    from graph_hscn.structure import Relation
    return Relation(ei.to(DEV), n, n)


def _csr_host(rel):
    c = rel.csr
    return c.rowptr.cpu().long(), c.col.cpu().long()[: rel.num_edges], c.eid.cpu().long()[: rel.num_edges]


def _spmm_f32_emulation(rowptr, col, w_slot, h, n):
    """The kernel's arithmetic on the CPU in float32: per row, acc = fl(acc + fl(w * h[col])) in CSR slot order."""
    deg = rowptr[1:] - rowptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(n), deg)
    rank = torch.arange(col.numel()) - rowptr[row_of]
    acc = torch.zeros(n, h.shape[1], dtype=torch.float32)
    for k in range(int(deg.max()) if n and col.numel() else 0):
        sel = rank == k
        r = row_of[sel]
        acc[r] = acc[r] + w_slot[sel].view(-1, 1) * h[col[sel]]
    return acc


def _spmm_refs(rowptr, col, w_slot, h, n):
    """float64 value, magnitude and per-row length; and the value with the single term removed that its row's
    bound sees best (largest |w h| relative to its row's bound)."""
    deg = rowptr[1:] - rowptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(n), deg)
    h64, w64 = h.double(), w_slot.double()
    terms = w64.view(-1, 1) * h64[col]
    ref = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add_(0, row_of, terms)
    mag = torch.zeros_like(ref).index_add_(0, row_of, terms.abs())
    nrow = (deg + 3).double().view(-1, 1)
    ratio = terms.abs() / (nrow[row_of] * mag[row_of] + 1e-300)
    k = int(ratio.argmax())
    e, f = divmod(k, h.shape[1])
    dropped = ref.clone()
    dropped[row_of[e], f] -= terms[e, f]
    return ref, mag, nrow, dropped


SPMM_WIDTHS = {"w4_pipe": 4, "w8_pipe": 8, "w16_pipe": 16, "w32_pipe": 32, "w10_vec1": 10, "w33_vec1": 33,
               "w64_nv2": 64, "w128_nv2": 128, "w256_nv2": 256}


@pytest.mark.parametrize("mode", ["gcn", "weighted"])
@pytest.mark.parametrize("wid", list(SPMM_WIDTHS), ids=list(SPMM_WIDTHS))
def test_spmm_f64_and_bitwise_cpu_order(wid, mode):
    """Degrees 0, 1, 2, 3, 4, 5, 8 (k_spmm_pipe carries four columns: 4/5 is its boundary) and one hub of 3000
    in-edges.  Bitwise equal to the float32 CPU evaluation in CSR order, and within the float64 bound."""
    width = SPMM_WIDTHS[wid]
    n = 700
    ei = _graph_with_degrees(n, 3000, width)
    rel = _rel(ei, n)
    rowptr, col, eid = _csr_host(rel)
    h = torch.randn(n, width, generator=_gen(width + 1))
    hd = h.to(DEV)
    if mode == "gcn":
        dinv = rel.dinv.cpu()
        row_of = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
        w_slot = dinv[col] * dinv[row_of]
        got = torch.empty(n, width, device=DEV)
        call("hscn_spmm_csr_gcn", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(rel.dinv), ptr(rel.dinv), ptr(hd), None,
             ptr(got), n, width, 0, 0, stream())
    else:
        wts = torch.randn(rel.num_edges, generator=_gen(width + 2))
        w_slot = wts[eid]
        got = torch.empty(n, width, device=DEV)
        wd = wts.to(DEV)
        call("hscn_spmm_csr_weighted", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(rel.csr.eid), ptr(wd),
             ptr(hd), ptr(got), n, width, stream())
    assert torch.equal(got.cpu(), _spmm_f32_emulation(rowptr, col, w_slot, h, n))
    ref, mag, nrow, dropped = _spmm_refs(rowptr, col, w_slot, h, n)
    check_f64(got, ref, mag, nrow, dropped, what=f"spmm {mode} {wid}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("wid", ["w16_pipe", "w10_vec1", "w128_nv2"])
def test_spmm_gcn_bias_accumulate_act(wid, act):
    width = SPMM_WIDTHS[wid]
    n = 500
    ei = _graph_with_degrees(n, 0, 5 * width)
    rel = _rel(ei, n)
    rowptr, col, _ = _csr_host(rel)
    g = _gen(width)
    h, bias, prev = torch.randn(n, width, generator=g), torch.randn(width, generator=g), torch.randn(n, width, generator=g)
    out = prev.to(DEV).contiguous()
    hd, bd = _dev(h, bias)
    call("hscn_spmm_csr_gcn", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(rel.dinv), ptr(rel.dinv), ptr(hd),
         ptr(bd), ptr(out), n, width, 1, ACT[act], stream())
    dinv = rel.dinv.cpu()
    row_of = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    w_slot = dinv[col] * dinv[row_of]
    if act in ("identity", "relu"):
        want = _act64(_spmm_f32_emulation(rowptr, col, w_slot, h, n) + bias + prev, act).float()
        assert torch.equal(out.cpu(), want)
    ref, mag, nrow, _ = _spmm_refs(rowptr, col, w_slot, h, n)
    pre = ref + bias.double() + prev.double()
    y = _act64(pre, act)
    mag = mag + bias.double().abs() + prev.double().abs() + y.abs()
    # the accumulated value is one term of its element: drop the one the bound sees best (among the elements whose
    # output it changes -- relu hides a term of an element that stays negative)
    seen = _act64(pre - prev.double(), act) != y
    k = int(torch.where(seen, prev.double().abs() / (mag * nrow), torch.zeros_like(y)).argmax())
    r, f = divmod(k, width)
    pre_d = pre.clone()
    pre_d[r, f] -= prev[r, f].double()
    check_f64(out, y, mag, nrow + 6, _act64(pre_d, act), what=f"spmm epilogue {wid} {act}")


def test_spmm_gridstride_past_block_cap():
    """width 16 (k_spmm_pipe, RPB 64): 600 k rows > 8192 blocks x 64 rows; every row of the tail bit-exact."""
    n, width = 600_000, 16
    g = _gen(77)
    d = torch.randint(0, 4, (n,), generator=g)
    dst = torch.repeat_interleave(torch.arange(n), d)
    ei = torch.stack([torch.randint(0, n, (dst.numel(),), generator=g), dst])
    rel = _rel(ei, n)
    rowptr, col, eid = _csr_host(rel)
    h = torch.randn(n, width, generator=g)
    wts = torch.randn(rel.num_edges, generator=g)
    got = torch.empty(n, width, device=DEV)
    wd, hd = _dev(wts, h)
    call("hscn_spmm_csr_weighted", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(rel.csr.eid), ptr(wd),
         ptr(hd), ptr(got), n, width, stream())
    assert torch.equal(got.cpu(), _spmm_f32_emulation(rowptr, col, wts[eid], h, n))


# --------------------------------------------------------------------------- #
# hscn_gat_segment_fwd
# --------------------------------------------------------------------------- #
GAT_WIDTHS = {"w1_vec1": 1, "w3_vec1": 3, "w5_vec1": 5, "w4": 4, "w64": 64, "w256_lprp64": 256}


def _gat_ref(rowptr, col, a_s, a_d, h, bias, prev, slope, act):
    n = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(n), deg)
    z = a_s.double()[col] + a_d.double()[row_of]
    z = torch.where(z > 0, z, z * slope)
    m = torch.full((n,), -math.inf, dtype=torch.float64).scatter_reduce(0, row_of, z, "amax")
    ex = torch.exp(z - m[row_of])
    den = torch.zeros(n, dtype=torch.float64).index_add_(0, row_of, ex) + 1e-16
    alpha = ex / den[row_of]
    terms = alpha.view(-1, 1) * h.double()[col]
    agg = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add_(0, row_of, terms)
    mag = torch.zeros_like(agg).index_add_(0, row_of, terms.abs())
    pre = agg.clone()
    for t in (bias, prev):
        if t is not None:
            pre = pre + t.double()
            mag = mag + t.double().abs()
    y = _act64(pre, act)
    mag = mag + y.abs()
    zmax = torch.zeros(n, dtype=torch.float64).scatter_reduce(0, row_of, z.abs(), "amax")
    kappa = (deg.double() + 8 + 2 * zmax + m.abs().nan_to_num(posinf=0.0, neginf=0.0)).view(-1, 1)
    ratio = terms.abs() / (kappa[row_of] * mag[row_of] + 1e-300)
    k = int(ratio.argmax()) if terms.numel() else 0
    e, f = divmod(k, h.shape[1])
    pre_d = pre.clone()
    if terms.numel():
        pre_d[row_of[e], f] -= terms[e, f]
    return y, mag, kappa, _act64(pre_d, act), alpha, row_of, kappa[row_of].view(-1)


def _gat_graph(nd, ns, seed):
    """destinations of in-degree 0, 1, 2, 5, 70 (> 64: the lanes stride the row) cycling, sources random."""
    g = _gen(seed)
    d = torch.tensor([0, 1, 2, 5, 70])[torch.arange(nd) % 5]
    dst = torch.repeat_interleave(torch.arange(nd), d)
    src = torch.randint(0, ns, (dst.numel(),), generator=g)
    return torch.stack([src, dst])


def _gat_call(rel, a_s, a_d, h, bias, out, width, slope, acc, act):
    alpha = torch.empty(max(rel.num_edges, 1), device=DEV)
    rc = _hip.lib().hscn_gat_segment_fwd(ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(a_s), ptr(a_d), ptr(h), ptr(bias),
                                         ptr(alpha), ptr(out), rel.num_dst, width, float(slope), acc, ACT[act],
                                         stream())
    return rc, alpha


@pytest.mark.parametrize("act,acc", [("identity", 0), ("elu", 1)])
@pytest.mark.parametrize("wid", list(GAT_WIDTHS), ids=list(GAT_WIDTHS))
def test_gat_segment_fwd(wid, act, acc):
    """Scores spread over +-100: exp overflows unless the row maximum is subtracted first."""
    from graph_hscn.structure import Relation
    width = GAT_WIDTHS[wid]
    nd, ns, slope = 400, 300, 0.2
    ei = _gat_graph(nd, ns, width)
    rel = Relation(ei.to(DEV), ns, nd)
    g = _gen(width + 5)
    a_s = (torch.rand(ns, generator=g) - 0.5) * 100
    a_d = (torch.rand(nd, generator=g) - 0.5) * 100
    h = torch.randn(ns, width, generator=g)
    bias = torch.randn(width, generator=g)
    prev = torch.randn(nd, width, generator=g) if acc else None
    out = prev.to(DEV).contiguous() if acc else torch.empty(nd, width, device=DEV)
    rc, alpha = _gat_call(rel, *_dev(a_s, a_d, h, bias), out, width, slope, acc, act)
    assert rc == 0
    rowptr, col, _ = _csr_host(rel)
    y, mag, kappa, dropped, alpha64, _, ka = _gat_ref(rowptr, col, a_s, a_d, h, bias, prev, slope, act)
    check_f64(out, y, mag, kappa, dropped, what=f"gat {wid} out")
    k = int(alpha64.argmax())
    adrop = alpha64.clone()
    adrop[k] = 0
    check_f64(alpha[: rel.num_edges], alpha64, alpha64, ka, adrop, tiny=1e-37, what=f"gat {wid} alpha")
    empty = (rowptr[1:] == rowptr[:-1]).nonzero().view(-1)
    base = bias.double().expand(nd, width) + (prev.double() if acc else 0)
    yb = _act64(base[empty], act)                   # a destination with no in-edges: act(bias (+ what was there))
    assert f64_close(out.cpu()[empty], yb, base[empty].abs() + yb.abs(), 8, what=f"gat {wid} empty rows")
    if not acc:
        assert torch.equal(out.cpu()[empty], _act64(bias.expand(len(empty), width), act)) or act != "identity"


def test_gat_segment_fwd_refuses_width_257_and_strides_past_block_cap():
    from graph_hscn.structure import Relation
    ei = _gat_graph(8, 8, 0)
    rel = Relation(ei.to(DEV), 8, 8)
    z = torch.zeros(8, device=DEV)
    h = torch.zeros(8, 257, device=DEV)
    out = torch.empty(8, 257, device=DEV)
    rc, _ = _gat_call(rel, z, z, h, None, out, 257, 0.2, 0, "identity")
    assert rc == _unsupported()
    nd = 8192 * 4 + 3001                                # past 8192 blocks of 4 waves: grid-stride over destinations
    ei = _gat_graph(nd, 5000, 1)
    rel = Relation(ei.to(DEV), 5000, nd)
    g = _gen(2)
    a_s, a_d, h = torch.randn(5000, generator=g), torch.randn(nd, generator=g), torch.randn(5000, 16, generator=g)
    out = torch.full((nd, 16), float("nan"), device=DEV)
    rc, _ = _gat_call(rel, *_dev(a_s, a_d, h), None, out, 16, 0.2, 0, "identity")
    assert rc == 0
    rowptr, col, _ = _csr_host(rel)
    y, mag, kappa, dropped, *_ = _gat_ref(rowptr, col, a_s, a_d, h, None, None, 0.2, "identity")
    check_f64(out, y, mag, kappa, dropped, tiny=1e-30, what="gat tail")


# --------------------------------------------------------------------------- #
# hscn_segment_mean_fwd / _bwd
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("width", [1, 3, 16, 64], ids=["w1_vec1", "w3_vec1", "w16_vec4", "w64_vec4"])
def test_segment_mean(width):
    """Empty segments, one segment of 120 000 rows, the rest small."""
    counts = torch.tensor([3, 0, 1, 120_000, 0, 7, 2, 0, 50])
    _segment_mean_case(counts, width, seed=width)


def test_segment_mean_gridstride_past_block_cap():
    counts = torch.randint(0, 4, (8192 * 4 + 777,), generator=_gen(1))
    _segment_mean_case(counts, 8, seed=0)


def _segment_mean_case(counts, width, seed):
    B = counts.numel()
    N = int(counts.sum())
    rowptr = torch.zeros(B + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(counts, 0).int()
    batch = torch.repeat_interleave(torch.arange(B), counts)
    x = torch.randn(N, width, generator=_gen(seed)) + 2.0
    out = torch.empty(B, width, device=DEV)
    rpd, xd = _dev(rowptr, x)
    call("hscn_segment_mean_fwd", ptr(rpd), None, ptr(xd), ptr(out), B, width, stream())
    cnt = counts.clamp_min(1).double().view(-1, 1)
    ref = torch.zeros(B, width, dtype=torch.float64).index_add_(0, batch, x.double()) / cnt
    mag = torch.zeros_like(ref).index_add_(0, batch, x.double().abs()) / cnt
    nseg = counts.double().view(-1, 1) + 3
    ratio = (x.double().abs() / cnt[batch]) / (nseg[batch] * mag[batch])
    r, f = divmod(int(ratio.argmax()), width)
    dropped = ref.clone()
    dropped[batch[r], f] -= x[r, f].double() / cnt[batch[r], 0]
    check_f64(out, ref, mag, nseg, dropped, what=f"segment mean w{width}")
    gout = torch.randn(B, width, generator=_gen(seed + 1))
    gx = torch.empty(N, width, device=DEV)
    bd, gd = _dev(batch, gout)
    call("hscn_segment_mean_bwd", ptr(rpd), ptr(bd), ptr(gd), ptr(gx), N, width, stream())
    gref = gout.double()[batch] / cnt[batch]
    k = int(gref.abs().argmax())
    gdrop = gref.clone().view(-1)
    gdrop[k] = 0
    check_f64(gx, gref, gref.abs(), 2, gdrop.view_as(gref), what=f"segment mean bwd w{width}")


# --------------------------------------------------------------------------- #
# LayerNorm / BatchNorm
# --------------------------------------------------------------------------- #
def _norm_input(N, H, seed):
    x = torch.randn(N, H, generator=_gen(seed))
    if H >= 3 and N >= 2:
        x[:, 1] = 0.75                                   # a constant column: variance 0
        x[:, 2] = 1e4 + torch.randn(N, generator=_gen(seed + 1))   # mean 1e4, std 1: a one-pass variance cancels
    return x


def _norm_ref(x, gamma, beta, dim, eps):
    x64 = x.double()
    mu = x64.mean(dim, keepdim=True)
    var = ((x64 - mu) ** 2).mean(dim, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    y = (x64 - mu) * rstd * gamma.double() + beta.double()
    mag = (x64.abs() + mu.abs()) * rstd * gamma.double().abs() + beta.double().abs()
    return y, mag, mu, var


@pytest.mark.parametrize("N,H", [(1, 16), (5, 1), (300, 3), (1000, 16), (64, 1024)],
                         ids=["n1", "h1", "h3", "chunks", "h1024"])
def test_layer_norm_fwd(N, H):
    from graph_hscn.nn.functional import LayerNormFn
    x = _norm_input(N, H, N + H)
    if H >= 3:
        x[0] = 1e4 + torch.randn(H, generator=_gen(5))    # a row with mean 1e4, std 1
        x[min(1, N - 1)] = 0.5 if N > 1 else x[0]         # a constant row
    g = _gen(H)
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    y = LayerNormFn.apply(*_dev(x, gamma, beta), 1e-5)
    ref, mag, mu, _ = _norm_ref(x, gamma, beta, 1, 1e-5)
    r, f = divmod(int((x.double() - mu).abs().argmax()), H)
    dropped = ref.clone()                                 # the element without its input: (0 - mu) rstd gamma + beta
    dropped[r, f] = ref[r, f] - x[r, f].double() / torch.sqrt(((x.double() - mu) ** 2).mean(1)[r] + 1e-5) * gamma[f]
    check_f64(y, ref, mag, H + 8, dropped, what=f"layer norm {N}x{H}")


def test_layer_norm_refuses_h1025():
    x = torch.zeros(2, 1025, device=DEV)
    gm = torch.ones(1025, device=DEV)
    m = torch.empty(2, device=DEV)
    rc = _hip.lib().hscn_layer_norm_fwd(ptr(x), ptr(gm), ptr(gm), ptr(x), ptr(m), ptr(m), 2, 1025, 1e-5, stream())
    assert rc != 0


@pytest.mark.parametrize("N,H", [(2, 1), (300, 3), (3000, 16), (40, 1024), (8192 * 256 // 16 + 1000, 16)],
                         ids=["h1", "h3", "chunks", "h1024", "total_past_grid_cap"])
def test_batch_norm_fwd_train_and_eval(N, H):
    from graph_hscn.nn.functional import BatchNormFn
    x = _norm_input(N, H, N + 3 * H)
    g = _gen(H + 1)
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    rm0, rv0 = torch.randn(H, generator=g), torch.rand(H, generator=g) + 0.5
    rm, rv = rm0.to(DEV).contiguous(), rv0.to(DEV).contiguous()
    mom, eps = 0.1, 1e-5
    y = BatchNormFn.apply(*_dev(x, gamma, beta), rm, rv, True, mom, eps)
    ref, mag, mu, var = _norm_ref(x, gamma, beta, 0, eps)
    depth = 256 + (N + 255) // 256 + 8                    # NR_CHUNK rows per partial, then the ordered fold
    r, f = divmod(int((x.double() - mu).abs().argmax()), H)
    dropped = ref.clone()
    dropped[r, f] = ref[r, f] - x[r, f].double() / torch.sqrt(var[0, f] + eps) * gamma[f]
    check_f64(y, ref, mag, depth + 8, dropped, what=f"batch norm train {N}x{H}")
    # running statistics: (1 - m) old + m batch (unbiased variance)
    rm_ref = (1 - mom) * rm0.double() + mom * mu.view(-1)
    unb = var.view(-1) * N / max(N - 1, 1)
    rv_ref = (1 - mom) * rv0.double() + mom * unb
    xmag = x.double().abs().mean(0)
    check_f64(rm, rm_ref, (1 - mom) * rm0.double().abs() + mom * xmag, depth + 4,
              rm_ref - (1 - mom) * rm0.double(), what="running mean")
    vmag = (1 - mom) * rv0.double() + mom * ((x.double().abs() + mu.abs()) ** 2).mean(0) * N / max(N - 1, 1)
    check_f64(rv, rv_ref, vmag, 2 * depth + 8, rv_ref - (1 - mom) * rv0.double(), what="running var")
    # eval: the running statistics just written
    ye = BatchNormFn.apply(*_dev(x, gamma, beta), rm, rv, False, mom, eps)
    rs = 1 / torch.sqrt(rv.cpu().double() + eps)
    rmd = rm.cpu().double()
    eref = (x.double() - rmd) * rs * gamma.double() + beta.double()
    emag = (x.double().abs() + rmd.abs()) * rs * gamma.double().abs() + beta.double().abs()
    edrop = eref.clone()
    edrop[r, f] -= x[r, f].double() * rs[f] * gamma[f]
    check_f64(ye, eref, emag, 8, edrop, what=f"batch norm eval {N}x{H}")


# --------------------------------------------------------------------------- #
# hscn_criterion_fwd / hscn_scale
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", [0, 1], ids=["bce_logits", "l1"])
@pytest.mark.parametrize("count", [1, 4095, 4096, 4097, 150_001])
def test_criterion(kind, count):
    g = _gen(count + kind)
    pred = torch.randn(count, generator=g) * 4
    pred[: min(count, 2)] = torch.tensor([80.0, -80.0])[: min(count, 2)]
    tgt = (torch.rand(count, generator=g) > 0.5).float() if kind == 0 else torch.randn(count, generator=g)
    loss = torch.empty(1, device=DEV)
    score = torch.empty(count, device=DEV)
    grad = torch.empty(count, device=DEV)
    pd, td = _dev(pred, tgt)
    call("hscn_criterion_fwd", ptr(pd), ptr(td), count, kind, ptr(loss), ptr(score), ptr(grad), stream())
    p, t = pred.double(), tgt.double()
    if kind == 0:
        li = p.clamp_min(0) - p * t + torch.log1p(torch.exp(-p.abs()))
        gi = (torch.sigmoid(p) - t) / count
        gmag = (torch.sigmoid(p) + t.abs()) / count
        lmag = p.clamp_min(0) + (p * t).abs() + torch.log1p(torch.exp(-p.abs()))
    else:
        li = (p - t).abs()
        gi = torch.sign(p - t) / count
        gmag = gi.abs()
        lmag = p.abs() + t.abs()
    ref = li.mean().view(1)
    lm = lmag.mean().view(1)
    # per thread a strided chain of <= ceil(count / 1024) terms, then 64 lanes, 16 waves: the tree's depth
    depth = (count + 1023) // 1024 + 6 + 4 + 8
    dropped = ref - li.max() / count
    check_f64(loss, ref, lm, depth, dropped, what=f"criterion {kind} {count}")
    k = int(gi.abs().argmax())
    gd = gi.clone()
    gd[k] = 0
    check_f64(grad, gi, gmag, 6, gd, what="criterion grad")
    sg = torch.sigmoid(p)
    sd = sg.clone()
    sd[int(sg.argmax())] = 0
    check_f64(score, sg, sg, 6, sd, tiny=1e-37, what="criterion score")
    s = torch.tensor([0.37], device=DEV)
    y = torch.empty(count, device=DEV)
    call("hscn_scale", ptr(s), ptr(grad), ptr(y), count, stream())
    yref = float(s) * grad.cpu().double()
    yd = yref.clone()
    yd[int(yref.abs().argmax())] = 0
    check_f64(y, yref, yref.abs(), 2, yd, tiny=1e-37, what="scale")


# --------------------------------------------------------------------------- #
# backward of GAT and of the norms, against float64 autograd
# --------------------------------------------------------------------------- #
def _grad_check(got, ref, dropped, n, what):
    """Composite backward chains (softmax, normalisation): the bound of ``f64_close`` with ``mag`` = the float64
    gradient's scale (max |ref| of the tensor, broadcast) and ``n`` = the longest sum feeding an element plus the
    op's condition -- the derivation of helpers.f64_close for non-linear ops, read normwise."""
    ref = ref.detach().cpu().double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    check_f64(got, ref, torch.full_like(ref, scale), n, dropped, what=what)


def _gat64(xs, xd, Ws, Wd, att_s, att_d, bias, src, dst, nd, slope, act):
    hs, hd = xs @ Ws.t(), xd @ Wd.t()
    z = (hs @ att_s)[src] + (hd @ att_d)[dst]
    z = torch.where(z > 0, z, z * slope)
    m = torch.full((nd,), -math.inf, dtype=torch.float64).scatter_reduce(0, dst, z.detach(), "amax")
    ex = torch.exp(z - m[dst])
    den = torch.zeros(nd, dtype=torch.float64).index_add(0, dst, ex) + 1e-16
    alpha = ex / den[dst]
    out = torch.zeros(nd, hs.shape[1], dtype=torch.float64).index_add(0, dst, alpha.view(-1, 1) * hs[src]) + bias
    return _act64(out, act)


@pytest.mark.parametrize("act", ["identity", "elu"])
@pytest.mark.parametrize("H", [3, 16, 64], ids=["w3_vec1", "w16", "w64"])
def test_gat_backward(H, act):
    """GATConvFn's backward (hscn_gat_segment_bwd_dst / _bwd_src, the linear weight gradients) against float64
    autograd; destinations of in-degree 0, 1, 2, 5, 70."""
    from graph_hscn.nn.functional import GATConvFn
    from graph_hscn.structure import Relation
    nd, ns, I, slope = 300, 200, 9, 0.2
    ei = _gat_graph(nd, ns, H + 11)
    rel = Relation(ei.to(DEV), ns, nd)
    g = _gen(H)
    xs, xd = torch.randn(ns, I, generator=g), torch.randn(nd, I, generator=g)
    Ws, Wd = torch.randn(H, I, generator=g) / 3, torch.randn(H, I, generator=g) / 3
    att_s, att_d, bias = torch.randn(H, generator=g), torch.randn(H, generator=g), torch.randn(H, generator=g)
    gy = torch.randn(nd, H, generator=g)
    leaves = [t.to(DEV).contiguous().requires_grad_() for t in (xs, xd, Ws, Wd, att_s.view(1, 1, H),
                                                                 att_d.view(1, 1, H), bias)]
    out = GATConvFn.apply(*leaves, rel, slope, ACT[act])
    out.backward(gy.to(DEV))
    src, dst = ei[0], ei[1]

    def grads(keep):
        l64 = [t.double().clone().requires_grad_() for t in (xs, xd, Ws, Wd, att_s, att_d, bias)]
        o = _gat64(*l64, src[keep], dst[keep], nd, slope, act)
        o.backward(gy.double())
        return [t.grad for t in l64], o.detach()

    ref, _ = grads(torch.ones(src.numel(), dtype=torch.bool))
    # teeth: the same gradients with the largest term of the upstream sums left out -- the largest |gy| among
    # destinations of in-degree >= 2 (a lone edge has alpha = 1 whatever its score: no attention gradient sees it)
    # (and of the least saturated softmax: a one-hot alpha hides a row from the attention gradients as well)
    with torch.no_grad():
        hs0 = xs.double() @ Ws.double().t()
        z0 = (hs0 @ att_s.double())[src] + ((xd.double() @ Wd.double().t()) @ att_d.double())[dst]
        z0 = torch.where(z0 > 0, z0, z0 * slope)
        m0 = torch.full((nd,), -math.inf, dtype=torch.float64).scatter_reduce(0, dst, z0, "amax")
        ex0 = torch.exp(z0 - m0[dst])
        a0 = ex0 / torch.zeros(nd, dtype=torch.float64).index_add(0, dst, ex0)[dst]
        spread = torch.zeros(nd, dtype=torch.float64).index_add(0, dst, a0 * (1 - a0))
    d_row = int(spread.argmax())
    gy_d = gy.clone()
    gy_d[d_row, int(gy[d_row].abs().argmax())] = 0
    l64 = [t.double().clone().requires_grad_() for t in (xs, xd, Ws, Wd, att_s, att_d, bias)]
    _gat64(*l64, src, dst, nd, slope, act).backward(gy_d.double())
    drop = [t.grad for t in l64]
    hs = xs.double() @ Ws.double().t()
    z = (hs @ att_s.double())[src] + ((xd.double() @ Wd.double().t()) @ att_d.double())[dst]
    n = 70 + I + 2 * H + 16 + 2 * float(z.abs().max())
    names = ["x_src", "x_dst", "W_src", "W_dst", "att_src", "att_dst", "bias"]
    for name, t, r, d in zip(names, leaves, ref, drop):
        got = t.grad.cpu().view(r.shape)
        if name in ("x_src", "W_src", "W_dst", "att_src", "att_dst"):
            n_t = n + (ns if name != "x_src" else 0) + nd * (name in ("W_dst", "att_dst"))
        else:
            n_t = n
        if name in ("x_dst", "W_dst", "att_dst"):
            # the destination side reaches the loss only through the softmax's derivative (sum_e alpha_e (h_e - out) . gy), where one
            # dropped term is damped below these tensors' normwise scale; the teeth of this test are the source side and the bias
            assert f64_close(got, r, torch.full_like(r, float(r.abs().max())), n_t, what=f"gat bwd {H} {act} {name}")
        else:
            _grad_check(got, r, d, n_t, f"gat bwd {H} {act} {name}")


@pytest.mark.parametrize("kind", ["layer", "batch"])
@pytest.mark.parametrize("N,H", [(1, 16), (300, 3), (3000, 16), (40, 1024)], ids=["n1", "h3", "chunks", "h1024"])
def test_norm_backward(kind, N, H):
    """hscn_layer_norm_bwd / hscn_batch_norm_bwd (k_col_partials + k_col_fold over NR_CHUNK-row chunks, k_bn_bwd_x)
    against float64 autograd; gbeta = sum gy is linear and gets the componentwise bound."""
    from graph_hscn.nn.functional import BatchNormFn, LayerNormFn
    if kind == "batch" and N == 1:
        N = 2
    x = _norm_input(N, H, N + H + 1)
    g = _gen(N * 3 + H)
    gamma, beta = torch.randn(H, generator=g), torch.randn(H, generator=g)
    gy = torch.randn(N, H, generator=g)
    xd, gd, bd = [t.to(DEV).contiguous().requires_grad_() for t in (x, gamma, beta)]
    if kind == "layer":
        y = LayerNormFn.apply(xd, gd, bd, 1e-5)
    else:
        rm, rv = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
        y = BatchNormFn.apply(xd, gd, bd, rm, rv, True, 0.1, 1e-5)
    y.backward(gy.to(DEV))

    def grads(gy_):
        l64 = [t.double().clone().requires_grad_() for t in (x, gamma, beta)]
        if kind == "layer":
            o = torch.nn.functional.layer_norm(l64[0], (H,), l64[1], l64[2], 1e-5)
        else:
            o = torch.nn.functional.batch_norm(l64[0], None, None, l64[1], l64[2], True, 0.1, 1e-5)
        o.backward(gy_.double())
        return [t.grad for t in l64]

    ref = grads(gy)
    x64 = x.double()
    dim = 1 if kind == "layer" else 0
    mu = x64.mean(dim, keepdim=True)
    rstd = 1 / torch.sqrt(((x64 - mu) ** 2).mean(dim, keepdim=True) + 1e-5)
    r, f = divmod(int((gy.double() * (x64 - mu) * rstd).abs().argmax()), H)   # (not in a constant column / row)
    gy_d = gy.clone()
    gy_d[r, f] = 0                                       # the largest single term of every sum it feeds
    drop = grads(gy_d)
    depth = (H if kind == "layer" else N) + 16
    cols = 256 + (N + 255) // 256 + 8                    # NR_CHUNK rows per partial, then the ordered fold
    _grad_check(xd.grad, ref[0], drop[0], depth + 8, f"{kind} norm bwd x {N}x{H}")
    gg_mag = (gy.double().abs() * (x64.abs() + mu.abs()) * rstd).sum(0)
    check_f64(gd.grad, ref[1], gg_mag, cols + depth, drop[1], what=f"{kind} norm bwd gamma")
    check_f64(bd.grad, ref[2], gy.double().abs().sum(0), cols, drop[2], what=f"{kind} norm bwd beta")


def test_batch_norm_refuses_h1025():
    x = torch.zeros(2, 1025, device=DEV)
    gm = torch.ones(1025, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    rc = _hip.lib().hscn_batch_norm_fwd(ptr(x), ptr(gm), ptr(gm), ptr(gm), ptr(gm), ptr(x), ptr(gm), ptr(gm), 2, 1025,
                                        1e-5, 0.1, 1, ptr(ws), ws.numel() * 4, stream())
    assert rc != 0


# --------------------------------------------------------------------------- #
# MinCUT: sparse, dense, ragged (float and byte adjacency); hscn_dense_adj_s; hscn_bgemm_f32
# --------------------------------------------------------------------------- #
def _mincut_graphs(sizes, seed):
    """Block-diagonal batch: every graph random symmetric edges plus one self loop per node (A + I, as stage A
    builds it), so a 1-node graph has degree 1."""
    g = _gen(seed)
    eis, off = [], 0
    for n in sizes:
        e = torch.randint(0, n, (2, 3 * n), generator=g)
        e = torch.cat([e, e.flip(0), torch.arange(n).repeat(2, 1)], 1)
        eis.append(e + off)
        off += n
    return torch.cat(eis, 1)


def _dense_blocks(ei, sizes, drop_edge=None):
    """float64 [n, n] adjacency of every graph; ``drop_edge``: one edge-list slot left out (the teeth)."""
    keep = torch.ones(ei.shape[1], dtype=torch.bool)
    if drop_edge is not None:
        keep[drop_edge] = False
    e = ei[:, keep]
    out, off = [], 0
    for n in sizes:
        sel = (e[0] >= off) & (e[0] < off + n)
        A = torch.zeros(n, n, dtype=torch.float64)
        A.index_put_((e[0, sel] - off, e[1, sel] - off), torch.ones(int(sel.sum()), dtype=torch.float64),
                     accumulate=True)
        out.append(A)
        off += n
    return out


def _mincut64(logits, x, blocks, sizes):
    """oracle.pyg_ops.dense_mincut_pool per graph in float64, losses averaged; gradient of 1.3 mc + 0.7 o."""
    from oracle import pyg_ops as P
    lg = logits.double().clone().requires_grad_()
    mcs, oos, pxs, off = [], [], [], 0
    for A, n in zip(blocks, sizes):
        xb = x[off:off + n].double() if x is not None else torch.zeros(n, 1, dtype=torch.float64)
        out, _, mc, oo = P.dense_mincut_pool(xb, A, lg[off:off + n])
        mcs.append(mc)
        oos.append(oo)
        pxs.append(out[0].detach())
        off += n
    mc, oo = torch.stack(mcs).mean(), torch.stack(oos).mean()
    (1.3 * mc + 0.7 * oo).backward()
    return float(mc.detach()), float(oo.detach()), pxs, lg.grad


def _mincut_grad_scale(logits, x, blocks, sizes):
    """Scale of the logits gradient before the softmax's cancellation: S (|G| + sum_k S |G|) with G = dL/dS, taken
    through a leaf S fed back as log S (softmax(log S) = S).  A 1-node graph's losses do not depend on S at all,
    so its gradient is 0 up to the rounding of terms of this size."""
    from oracle import pyg_ops as P
    S = torch.softmax(logits.double(), 1).requires_grad_()
    mcs, oos, off = [], [], 0
    for A, n in zip(blocks, sizes):
        xb = x[off:off + n].double() if x is not None else torch.zeros(n, 1, dtype=torch.float64)
        _, _, mc, oo = P.dense_mincut_pool(xb, A, torch.log(S[off:off + n]))
        mcs.append(mc)
        oos.append(oo)
        off += n
    (1.3 * torch.stack(mcs).mean() + 0.7 * torch.stack(oos).mean()).backward()
    SG = S.detach() * S.grad.abs()
    return float((SG + S.detach() * SG.sum(1, keepdim=True)).max())


def _mincut_check(route, S, mc, oo, px, glog, logits, x, ei, sizes, K):
    n_max = max(sizes)
    depth = 2 * n_max + 2 * K + 32                       # A S, then S^T (A S) and its trace / S^T D S
    depth_o = n_max + K * K + 32                          # S^T S, then its Frobenius norms
    blocks = _dense_blocks(ei, sizes)
    mc64, oo64, px64, g64 = _mincut64(logits, x, blocks, sizes)
    # S = softmax(logits): relative error ~ u (K + |l - max l|); teeth: the largest exp term left out of a row's sum
    l64 = logits.double()
    S64 = torch.softmax(l64, 1)
    i = int(S64.max(1).values.argmax())
    Sd = S64.clone()
    Sd[i] = S64[i] / (1 - S64[i].max())
    spread = float((l64 - l64.max(1, keepdim=True).values).abs().max())
    check_f64(S, S64, S64, K + 8 + spread, Sd, tiny=1e-37, what=f"{route} S K={K}")
    # losses: ratios / norms of sums of <= depth non-negative terms
    assert f64_close(torch.tensor([float(mc)]), torch.tensor([mc64]), abs(mc64) + 1e-30, depth, what=f"{route} mc")
    assert f64_close(torch.tensor([float(oo)]), torch.tensor([oo64]), 1.0, depth_o, what=f"{route} ortho")
    sc = max(float(g64.abs().max()), _mincut_grad_scale(logits, x, blocks, sizes))
    if n_max == 1:
        # every loss term is S-independent: the gradient is 0 up to the rounding of the cancelling terms, each at most
        # 2 K (1.3 + 0.7) / B in size (s / (s . s) <= K |s| for the mincut ratio, likewise for the ortho norm)
        sc = max(sc, 2 * K * 2.0 / len(sizes))
    scale = torch.full_like(g64, sc)
    if K > 1 and n_max > 1:                              # (a 1-node graph's mincut is -1 whatever its loops)
        # teeth: the same values with the adjacency entry of the largest term s_i . s_j left out
        src, dst = ei[0], ei[1]
        e = int((S64[src] * S64[dst]).sum(1).argmax())
        mcd, _, _, gd = _mincut64(logits, x, _dense_blocks(ei, sizes, e), sizes)
        assert not f64_close(torch.tensor([float(mc)]), torch.tensor([mcd]), abs(mc64), depth)
        check_f64(glog, g64, scale, depth + spread, gd, what=f"{route} grad K={K}")
    else:
        assert f64_close(glog, g64, scale, depth, tiny=1e-30, what=f"{route} grad K=1")
    if x is not None and px is not None:
        off = 0
        for b, n in enumerate(sizes):
            Sb = S64[off:off + n]
            xb = x[off:off + n].double()
            dropped = drop_largest_product(px64[b], Sb.t(), xb)
            check_f64(px[b, :, : x.shape[1]].cpu() if px.dim() == 3 else px, px64[b], Sb.t() @ xb.abs(), n + 8,
                      dropped, what=f"{route} pooled x graph {b}")
            off += n


MINCUT_K = {"k1": 1, "k2": 2, "k5": 5, "k64": 64}


@pytest.mark.parametrize("Fx", [0, 7], ids=["fx0", "fx7"])
@pytest.mark.parametrize("kk", list(MINCUT_K) + ["k128_lds_over_64k"])
def test_mincut_sparse(kk, Fx):
    from graph_hscn.nn.functional import MinCutSparseFn
    from graph_hscn.structure import Relation
    K = 128 if kk.startswith("k128") else MINCUT_K[kk]
    sizes = [1, 37, 100, 130]
    ei = _mincut_graphs(sizes, K + Fx)
    N = sum(sizes)
    g = _gen(K * 3 + Fx)
    logits = torch.randn(N, K, generator=g) * 2
    x = torch.randn(N, Fx, generator=g) if Fx else None
    rel = Relation(ei.to(DEV), N, N)
    nptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    ld = logits.to(DEV).requires_grad_()
    xd = x.to(DEV) if x is not None else None
    S, mc, oo, px, _ = MinCutSparseFn.apply(ld, xd, rel, nptr, len(sizes))
    (1.3 * mc + 0.7 * oo).backward()
    _mincut_check("sparse", S.cpu(), mc, oo, px.cpu() if px is not None else None, ld.grad.cpu(), logits, x, ei,
                  sizes, K)


@pytest.mark.parametrize("K", [82, 83, 112, 113])
def test_mincut_sparse_at_the_lds_opt_in_line(K):
    """Without x, k_mincut_stats asks for (2 K^2 + 34 K + 20) * 4 bytes of LDS and k_mincut_bwd for (K^2 + 32 K + 4) * 4:
    K = 82 is the last width whose forward stays within the 64 KB a launch gets unasked and 83 the first that opts in;
    112 / 113 are the same pair for the backward.  Two small graphs; the float64 referee of test_mincut_sparse."""
    from graph_hscn.nn.functional import MinCutSparseFn
    from graph_hscn.structure import Relation
    sizes = [5, 20]
    ei = _mincut_graphs(sizes, K)
    N = sum(sizes)
    logits = torch.randn(N, K, generator=_gen(K * 3)) * 2
    rel = Relation(ei.to(DEV), N, N)
    nptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    ld = logits.to(DEV).requires_grad_()
    S, mc, oo, px, _ = MinCutSparseFn.apply(ld, None, rel, nptr, len(sizes))
    (1.3 * mc + 0.7 * oo).backward()
    _mincut_check("sparse", S.cpu(), mc, oo, None, ld.grad.cpu(), logits, None, ei, sizes, K)


def test_mincut_sparse_refuses_k256():
    """K = 256 passes the argument check but its 2 K^2 cluster-space floats exceed the 160 KiB LDS: refused."""
    from graph_hscn.structure import Relation
    sizes = [5]
    ei = _mincut_graphs(sizes, 0)
    rel = Relation(ei.to(DEV), 5, 5)
    K = 256
    lg = torch.randn(5, K, device=DEV)
    S = torch.empty_like(lg)
    stats, ss = torch.empty(1, 4, device=DEV), torch.empty(1, K, K, device=DEV)
    padj, losses = torch.empty(1, K, K, device=DEV), torch.empty(2, device=DEV)
    nptr = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    rc = _hip.lib().hscn_mincut_sparse_fwd(ptr(lg), None, ptr(rel.csr_t.rowptr), ptr(rel.csr_t.col), ptr(nptr), ptr(S),
                                           ptr(stats), ptr(ss), None, ptr(padj), ptr(losses), 5, 1, K, 0, stream())
    assert rc == _unsupported()


@pytest.mark.parametrize("Fx", [0, 7], ids=["fx0", "fx7"])
@pytest.mark.parametrize("kk", list(MINCUT_K))
@pytest.mark.parametrize("n", [1, 37, 100], ids=["n1", "n37_off_tile", "n100"])
def test_mincut_dense(n, kk, Fx):
    from graph_hscn.nn.functional import MinCutDenseFn
    from graph_hscn.nn.pool import to_dense_adj_batched
    K, B = MINCUT_K[kk], 3
    sizes = [n] * B
    ei = _mincut_graphs(sizes, n + K + Fx)
    g = _gen(n * 5 + K + Fx)
    logits = torch.randn(n * B, K, generator=g) * 2
    x = torch.randn(n * B, Fx, generator=g) if Fx else None
    adj = to_dense_adj_batched(ei.to(DEV), B, n)
    ld = logits.to(DEV).view(B, n, K).requires_grad_()
    xd = x.to(DEV).view(B, n, Fx) if x is not None else None
    S, mc, oo, px, _ = MinCutDenseFn.apply(ld, xd, adj)
    (1.3 * mc + 0.7 * oo).backward()
    _mincut_check("dense", S.cpu().view(-1, K), mc, oo, px.cpu() if px is not None else None,
                  ld.grad.cpu().view(-1, K), logits, x, ei, sizes, K)


@pytest.mark.parametrize("adj_kind", ["f32", "u8", "u8_sym"])
@pytest.mark.parametrize("Fx", [0, 7], ids=["fx0", "fx7"])
@pytest.mark.parametrize("kk", list(MINCUT_K))
def test_mincut_dense_ragged(kk, Fx, adj_kind):
    """Graphs of 1, 37, 100 and 130 nodes in one [B, 130, 130] adjacency: float, bytes, and bytes with the
    symmetry flags (the backward then takes A^T S from the forward's A S)."""
    from graph_hscn.nn.functional import MinCutDenseRaggedFn
    from graph_hscn.nn.pool import to_dense_adj_ragged
    K = MINCUT_K[kk]
    sizes = [1, 37, 100, 130]
    ei = _mincut_graphs(sizes, 7 * K + Fx)
    N, B, nmax = sum(sizes), len(sizes), max(sizes)
    g = _gen(K + 11 * Fx)
    logits = torch.randn(N, K, generator=g) * 2
    x = torch.randn(N, Fx, generator=g) if Fx else None
    nptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    gid = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    asym = None
    if adj_kind == "f32":
        adj = to_dense_adj_ragged(ei.to(DEV), nptr, gid, B, nmax)
    elif adj_kind == "u8":
        adj = to_dense_adj_ragged(ei.to(DEV), nptr, gid, B, nmax, as_bytes=True)
    else:
        adj, asym = to_dense_adj_ragged(ei.to(DEV), nptr, gid, B, nmax, as_bytes=True, symmetry=True)
        assert int(asym.sum()) == 0
    ld = logits.to(DEV).requires_grad_()
    xd = x.to(DEV) if x is not None else None
    S, mc, oo, px, _ = MinCutDenseRaggedFn.apply(ld, xd, adj, nptr, gid, asym)
    (1.3 * mc + 0.7 * oo).backward()
    _mincut_check(f"ragged {adj_kind}", S.cpu(), mc, oo, px.cpu() if px is not None else None, ld.grad.cpu(),
                  logits, x, ei, sizes, K)


@pytest.mark.parametrize("transA", [0, 1])
@pytest.mark.parametrize("elem", [4, 1], ids=["f32_adj", "u8_adj"])
@pytest.mark.parametrize("kk", list(MINCUT_K))
def test_dense_adj_s(kk, elem, transA):
    """hscn_dense_adj_s: A S (and deg = A 1) or A^T S per graph of a ragged batch, graphs of 1..130 nodes."""
    from graph_hscn.nn.pool import to_dense_adj_ragged
    K = MINCUT_K[kk]
    sizes = [1, 37, 100, 130]
    g = _gen(K + elem + 3 * transA)
    eis, off = [], 0
    for n in sizes:                                              # directed edges: A != A^T
        eis.append(torch.randint(0, n, (2, 4 * n), generator=g) + off)
        off += n
    ei = torch.cat(eis, 1)
    N, B, nmax = off, len(sizes), max(sizes)
    nptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    gid = torch.repeat_interleave(torch.arange(B, dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    adj = to_dense_adj_ragged(ei.to(DEV), nptr, gid, B, nmax, as_bytes=elem == 1)
    S = torch.randn(N, K, generator=g)
    Sd = S.to(DEV)
    out = torch.empty(N, K, device=DEV)
    deg = torch.empty(N, device=DEV)
    call("hscn_dense_adj_s", ptr(adj), elem, ptr(Sd), ptr(nptr), B, nmax, K, transA, ptr(out),
         ptr(deg) if not transA else None, stream())
    blocks = _dense_blocks(ei, sizes)
    ref, mag, drops, off = [], [], [], 0
    for A, n in zip(blocks, sizes):
        A = A.t() if transA else A
        Sb = S[off:off + n].double()
        ref.append(A @ Sb)
        mag.append(A @ Sb.abs())
        off += n
    ref, mag = torch.cat(ref), torch.cat(mag)
    b = 3                                                        # teeth in the largest graph
    o3 = sum(sizes[:b])
    A3 = blocks[b].t() if transA else blocks[b]
    dropped = ref.clone()
    dropped[o3:] = drop_largest_product(ref[o3:], A3, S[o3:].double())
    check_f64(out, ref, mag, nmax + 4, dropped, what=f"adj_s K={K} elem={elem} transA={transA}")
    if not transA:
        assert torch.equal(deg.cpu().double(), torch.cat([A.sum(1) for A in blocks]))


@pytest.mark.parametrize("M,N,Kd,ta", [(64, 16, 64, 0), (70, 33, 45, 0), (37, 64, 129, 1), (16, 5, 7, 1), (1, 1, 1, 0)],
                         ids=["tile", "off_tile", "transA_off_tile", "transA_small", "one"])
def test_bgemm_f32(M, N, Kd, ta):
    g = _gen(M + N + Kd)
    A = torch.randn(2, Kd, M, generator=g) if ta else torch.randn(2, M, Kd, generator=g)
    Bm = torch.randn(2, Kd, N, generator=g)
    Ad, Bd = _dev(A, Bm)
    C = torch.empty(2, M, N, device=DEV)
    call("hscn_bgemm_f32", ptr(Ad), ptr(Bd), ptr(C), 2, M, N, Kd, Ad.stride(1), N, N, Ad.stride(0), Kd * N, M * N, ta,
         stream())
    A64 = (A.transpose(1, 2) if ta else A).double()
    ref = A64 @ Bm.double()
    mag = A64.abs() @ Bm.double().abs()
    dropped = ref.clone()
    dropped[1] = drop_largest_product(ref[1], A64[1], Bm[1].double())
    check_f64(C, ref, mag, Kd + 4, dropped, what=f"bgemm {M}x{N}x{Kd} ta={ta}")


# --------------------------------------------------------------------------- #
# byte adjacency: saturation instead of a carry
# --------------------------------------------------------------------------- #
def _u8_batch(parallel):
    """Two graphs of 5 and 3 nodes (nmax 5, rows padded to 32 bytes): graph 0 has `parallel` copies of the edge
    (0 -> 1) and a single (0 -> 3); its entry (0, 2) -- the right-hand neighbour of (0, 1) -- and the last real
    column (0, 4) have no edge."""
    ei = torch.tensor([[0] * parallel + [0, 5, 6], [1] * parallel + [3, 6, 7]])
    nptr = torch.tensor([0, 5, 8], dtype=torch.int32)
    gid = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1], dtype=torch.int32)
    return ei, nptr, gid


@pytest.mark.parametrize("parallel", [255, 300])
def test_dense_adj_ragged_u8_saturates_without_carry(parallel):
    from graph_hscn.nn.pool import to_dense_adj_ragged
    ei, nptr, gid = _u8_batch(parallel)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    adj8 = to_dense_adj_ragged(ei.to(DEV), nptr.to(DEV), gid.to(DEV), 2, 5, as_bytes=True, flag=flag)
    a = adj8.cpu().long()
    want = torch.zeros_like(a)
    want[0, 0, 1] = min(parallel, 255)
    want[0, 0, 3] = 1
    want[1, 0, 1] = 1
    want[1, 1, 2] = 1
    assert a[0, 0, 1] == min(parallel, 255)
    assert a[0, 0, 2] == 0 and a[0, 0, 4] == 0 and int(a[0, 0, 5:].abs().sum()) == 0
    assert torch.equal(a, want)                                  # no other entry, no padding byte changed
    assert (int(flag.item()) & 16) == (16 if parallel > 255 else 0)


def test_scn_dense_byte_route_reports_saturation():
    """Through the model: 300 parallel edges either give the float64 oracle's losses or are reported -- the byte
    route saturates, so check_adjacency() must raise; the float adjacency gives the oracle's losses."""
    from graph_hscn.model.hscn import SCN
    from oracle import models as OM
    from oracle import pyg_ops as P
    ei, nptr, gid = _u8_batch(300)
    ei = torch.cat([ei, ei.flip(0)], 1)
    N, K = 8, 3
    torch.manual_seed(0)
    o = OM.SCN([16], "elu", 4, K)
    m = SCN([16], "elu", 4, K, mincut_route="dense").to(DEV)
    m.load_state_dict(o.state_dict())
    x = torch.randn(N, 4, generator=_gen(4))
    from graph_hscn.nn.pool import gcn_norm
    eid, ew = gcn_norm(ei.to(DEV), None, N, add_self_loops=True)
    m.check_adjacency()
    _, mc, oo, _ = m(x.to(DEV), eid, ew, node_ptr=nptr.to(DEV), nodes_per_graph=5, node_graph=gid.to(DEV),
                     raw_edge_index=ei.to(DEV))
    # float64 oracle: every graph's SCN on its own edge list (parallel edges counted), losses averaged
    od = copy.deepcopy(o).double()
    ref = _scn_losses_f64(od, x.double(), ei, [(0, 5), (5, 8)])
    got = (float(mc), float(oo))
    matches = all(abs(a - b) <= 1e-5 * max(1.0, abs(b)) for a, b in zip(got, ref))
    if not matches:
        with pytest.raises(OverflowError):
            m.check_adjacency()
    m.check_adjacency()                                          # a check clears the flag: the next one passes
    os.environ["HSCN_DENSE_ADJ"] = "f32"
    try:
        m2 = SCN([16], "elu", 4, K, mincut_route="dense").to(DEV)
        m2.load_state_dict(o.state_dict())
        _, mc2, oo2, _ = m2(x.to(DEV), eid, ew, node_ptr=nptr.to(DEV), nodes_per_graph=5, node_graph=gid.to(DEV),
                            raw_edge_index=ei.to(DEV))
        m2.check_adjacency()
    finally:
        del os.environ["HSCN_DENSE_ADJ"]
    assert abs(float(mc2) - ref[0]) <= 1e-5 and abs(float(oo2) - ref[1]) <= 1e-5


def _scn_losses_f64(od, x, ei, spans):
    from oracle import pyg_ops as P
    mcs, oos = [], []
    with torch.no_grad():
        for s0, s1 in spans:
            sel = (ei[0] >= s0) & (ei[0] < s1)
            eg, wg = P.gcn_norm(ei[:, sel] - s0, None, s1 - s0, add_self_loops=True)
            h = od.mp(x[s0:s1], eg, wg.double())                  # oracle/models.py SCN.forward, in float64
            adj = P.to_dense_adj(eg, s1 - s0).double()
            _, _, mc, oo = P.dense_mincut_pool(h, adj, od._run_mlp(h))
            mcs.append(float(mc))
            oos.append(float(oo))
    return sum(mcs) / len(mcs), sum(oos) / len(oos)


# --------------------------------------------------------------------------- #
# environment-selected variants: fresh child processes
# --------------------------------------------------------------------------- #
VARIANTS = [
    ({"HSCN_LINEAR_BWD_W": "0"}, "test_linear_bwd_w"),
    ({"HSCN_SPMM_PIPE": "0"}, "test_spmm"),
    ({"HSCN_SPMM_PIPE": "2"}, "test_spmm"),
    ({"HSCN_SPMM_NV": "1"}, "test_spmm_f64"),
    ({"HSCN_SPMM_NV": "4"}, "test_spmm_f64"),
    ({"HSCN_SPMM_PASSES": "2"}, "test_spmm"),
    ({"HSCN_DENSE_AS": "16"}, "mincut or dense_adj_s"),
    ({"HSCN_DENSE_AS": "32"}, "mincut or dense_adj_s"),
    ({"HSCN_DENSE_ROWS": "128"}, "mincut or dense_adj_s"),
    ({"HSCN_DENSE_ROWS": "256"}, "mincut or dense_adj_s"),
]


def test_environment_variants_in_child_processes():
    """Each switch is read once per process (static locals in the host code): run the matching cases of this file
    in a fresh interpreter per variant, one at a time, and stop at the first that fails.  The spmm variants meet the
    same bitwise CPU-order assertion as the default; HSCN_LINEAR_BWD_W=0 (the scalar partial kernel) the float64
    bound."""
    if os.environ.get("HSCN_F64_CHILD"):
        pytest.skip("inside a variant child")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env_add, sel in VARIANTS:
        env = dict(os.environ, HSCN_F64_CHILD="1", **env_add)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                            os.path.join("tests", "test_gpu_ops_f64.py"), "-k", f"({sel}) and not gridstride"],
                           cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{env_add}: child exited {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-2000:]}"
