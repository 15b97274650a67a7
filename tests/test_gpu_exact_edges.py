"""The structure and data-path kernels -- CSR builds, degree norms, dense adjacencies, argmax, the hetero build, the
device collate and the dropout generator -- bit for bit at their branch and loop-trip edges.

These kernels have exact answers: every assertion here is equality of integers, or of float32 values viewed as
int32.  No tolerance appears anywhere in this module.  References are plain numpy / Python written here, the host
transform ``graph_hscn/loader/hetero_data.py``, ``HeteroBatch.from_data_list`` and ``Tensor.max`` on the CPU.
Each section starts with the list of branches and loop edges read from the host dispatch and the kernel, and the case
that reaches each.  GPU tests carry the ``gpu`` mark one by one: the known-answer test of the Philox reference runs
without a device."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import DEV

gpu = pytest.mark.gpu

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3          # include/hscn.h: HSCN_E_*
INT32_MAX = 2 ** 31 - 1
LL, VV, LV = ("local", "to", "local"), ("virtual", "to", "virtual"), ("local", "to", "virtual")


def _bits(t):
    """float32 values as int32 bit patterns (numpy)."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def _same_floats(got, want):
    """Bitwise equality of two float32 arrays; two NaNs count as equal whatever their sign / payload bits."""
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
        return False
    ok = ~np.isnan(w)
    return np.array_equal(_bits(g)[ok], _bits(w)[ok])


def _lib():
    from graph_hscn import _hip
    return _hip.lib()


def _p(t):
    from graph_hscn import _hip
    return _hip.ptr(t)


def _stream():
    from graph_hscn import _hip
    return _hip.stream()


# ===================================================================================================================
# 1. CSR builds: hscn_csr_build, hscn_csr_build_pair, hscn_csr_cross_positions (csrc/structure.hip)
#
# Refusals before any launch (both builds): E < 0, rows < 0, NULL rowptr / workspace, NULL key / other / col / eid
# with E > 0 -> BADARG; E > INT32_MAX, rows >= INT32_MAX, (single build) cols > INT32_MAX -> UNSUPPORTED; workspace
# smaller than *_workspace_bytes -> WORKSPACE.  [test_refusals_csr]
# hscn_csr_build, with n1 = rows + 1 entries to scan:
#   * E == 0 skips k_hist / k_fill / k_rank: rowptr all zero.                        [rows 0, 1, 7, 5000, 9000; E = 0]
#   * n1 <= 8192: k_scan_single, one block, 4096 entries per trip with a carry between trips:
#       one trip  n1 <= 4096                                                         [rows 1, 50, 4095 (n1 = 4096)]
#       two trips 4096 < n1 <= 8192 (the carry)                                      [rows 4096 (n1 = 4097), 6000, 8191]
#   * n1 > 8192: k_scan_partial / k_scan_blocksums / k_scan_final over tiles of SCAN_TILE = 2048:
#       first size past the switch                                                   [rows 8192 (n1 = 8193): 5 tiles]
#       n1 a multiple of the tile, and one past it                                   [rows 10239 (n1 = 5 * 2048), 10240]
#       k_scan_blocksums' own loop, 1024 tiles per trip with a carry                 [rows 2097151 (1024 tiles, one
#                                                                                     trip), 2097152 (1025 tiles)]
#   * k_hist / k_fill / k_rank: one thread per edge, blocks of 256                   [E = 0, 1, 255, 256, 257, ...]
#       an endpoint outside [0, rows) x [0, cols): flag |= 1, the edge is in no array  [test_csr_out_of_range, at the
#                                                                                     one-trip, two-trip and three-launch
#                                                                                     size classes]
#       k_rank walks the whole row per edge                                          [hub: 20000 edges into one row;
#                                                                                     single row; single column]
#   * rows != cols (the key range and the other range are checked separately)        [bipartite, larger side either way]
# hscn_csr_build_pair: always the three-launch scan, grid (max(tiles_dst, tiles_src), 2); the blocks of the shorter
#   side beyond its own tiles return early; k_scan_blocksums_pair derives the tile count per side:
#       one tile on both sides                                                       [rows 1 .. 2047]
#       n1 = 2048 / 2049 (one tile / two tiles)                                      [rows 2047, 2048]
#       sides of different tile counts, either side longer                           [bipartite 9000 x 700, 700 x 9000,
#                                                                                     70000 x 3]
#       more than 1024 tiles                                                         [rows 2097152]
#       E == 0 (k_zero_pair and the scans only)                                      [E = 0 cases]
#   The pair must equal the two single builds array for array.                       [every case]
# hscn_csr_cross_positions: E == 0 returns before a launch; otherwise one thread per slot: pos_t = inv(eid)[eid_t]
#                                                                                    [every case with E > 0, E up to 40000]
# ===================================================================================================================
def _ref_csr(key, other, rows, cols):
    """Stable CSR of the in-range edges: numpy stable argsort + bincount."""
    ok = (key >= 0) & (key < rows) & (other >= 0) & (other < cols)
    idx = np.flatnonzero(ok)
    order = idx[np.argsort(key[idx], kind="stable")]
    rowptr = np.zeros(rows + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(key[idx], minlength=rows))
    return rowptr, other[order], order, bool((~ok).any())


def _check_csr(csr, key, other, rows, cols):
    rowptr, col, eid, bad = _ref_csr(key, other, rows, cols)
    m = int(rowptr[-1])
    assert np.array_equal(csr.rowptr.cpu().numpy().astype(np.int64), rowptr)
    assert np.array_equal(csr.eid.cpu().numpy()[:m].astype(np.int64), eid)
    assert np.array_equal(csr.col.cpu().numpy()[:m].astype(np.int64), col)
    assert int(csr.flag.item()) == (1 if bad else 0)


def _check_both_builds(src, dst, ns, nd):
    """Single builds (keyed by target, keyed by source) against numpy, the pair build against the single builds,
    cross positions against the inverse permutation."""
    from graph_hscn import _hip
    from graph_hscn.structure import build_csr, build_csr_pair
    s, d = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    a = build_csr(d, s, nd, ns)
    a_t = build_csr(s, d, ns, nd)
    b, b_t = build_csr_pair(s, d, ns, nd)
    torch.cuda.synchronize()
    _check_csr(a, dst, src, nd, ns)
    _check_csr(a_t, src, dst, ns, nd)
    m = int(a.rowptr[-1].item())
    for x, y in ((a, b), (a_t, b_t)):
        assert torch.equal(x.rowptr, y.rowptr)
        assert torch.equal(x.col[:m], y.col[:m]) and torch.equal(x.eid[:m], y.eid[:m])
    assert int(b.flag.item()) == int(a.flag.item())
    E = int(src.shape[0])
    if E and m == E:
        inv = torch.empty(E, dtype=torch.int32, device=DEV)
        pos = torch.empty(E, dtype=torch.int32, device=DEV)
        _hip.call("hscn_csr_cross_positions", _hip.ptr(a.eid), _hip.ptr(a_t.eid), E, _hip.ptr(inv), _hip.ptr(pos),
                  _hip.stream())
        want_inv = np.empty(E, dtype=np.int64)
        want_inv[a.eid.cpu().numpy()] = np.arange(E)
        assert np.array_equal(inv.cpu().numpy(), want_inv)
        assert np.array_equal(pos.cpu().numpy(), want_inv[a_t.eid.cpu().numpy()])


_CSR_SIZES = [(0, 0), (1, 0), (1, 1), (7, 0), (50, 255), (50, 256), (50, 257), (2047, 6000), (2048, 6000), (4094, 9000),
              (4095, 9000), (4096, 9000), (5000, 0), (6000, 20000), (8191, 20000), (8192, 20000), (9000, 0),
              (10239, 30000), (10240, 30000), (2097151, 5000), (2097152, 5000)]


@gpu
@pytest.mark.parametrize("n,E", _CSR_SIZES)
def test_csr_builds_at_every_scan_edge(n, E):
    rng = np.random.default_rng(n * 7 + E)
    hi = max(n, 1)
    src, dst = rng.integers(0, hi, E), rng.integers(0, hi, E)       # self loops and parallel edges included
    if E and n > 4096:
        # edges in the last rows and in the first: a lost carry or tile offset shows in every later rowptr entry
        dst[: E // 8] = rng.integers(0, 64, E // 8)
        dst[E // 8: E // 4] = n - 1 - rng.integers(0, 64, E // 4 - E // 8)
        src[: E // 8] = n - 1 - rng.integers(0, 64, E // 8)
        src[E // 8: E // 4] = rng.integers(0, 64, E // 4 - E // 8)
    _check_both_builds(src.astype(np.int64), dst.astype(np.int64), n, n)


def _constructed(case):
    rng = np.random.default_rng(11)
    if case == "hub":                 # 20000 edges into row 4100 of 8300 (three-launch scan), the rest random
        n = 8300
        src = np.concatenate([rng.integers(0, n, 20000), rng.integers(0, n, 3000)])
        dst = np.concatenate([np.full(20000, 4100), rng.integers(0, n, 3000)])
        p = rng.permutation(src.shape[0])
        return src[p], dst[p], n, n
    if case == "single_row":          # every edge has the same target: one row of the target-keyed CSR
        return rng.integers(0, 5000, 6000), np.full(6000, 4999), 5000, 5000
    if case == "single_column":       # every edge has the same source
        return np.zeros(6000, dtype=np.int64), rng.integers(0, 5000, 6000), 5000, 5000
    if case == "src_larger":
        return rng.integers(0, 9000, 15000), rng.integers(0, 700, 15000), 9000, 700
    if case == "dst_larger":
        return rng.integers(0, 700, 15000), rng.integers(0, 9000, 15000), 700, 9000
    if case == "three_targets":       # 70000 sources (35 tiles), 3 targets (one tile)
        return rng.integers(0, 70000, 40000), rng.integers(0, 3, 40000), 70000, 3
    if case == "one_target_no_edges":
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 9000, 1
    raise KeyError(case)


@gpu
@pytest.mark.parametrize("case", ["hub", "single_row", "single_column", "src_larger", "dst_larger", "three_targets",
                                  "one_target_no_edges"])
def test_csr_builds_on_constructed_graphs(case):
    src, dst, ns, nd = _constructed(case)
    _check_both_builds(src.astype(np.int64), dst.astype(np.int64), ns, nd)


@gpu
@pytest.mark.parametrize("n", [50, 3000, 6000, 9000, 70000])
def test_csr_out_of_range(n):
    """Endpoints outside the node range raise the flag and are absent from every array, at each size class of the
    scan; the edges that remain keep their stable order."""
    rng = np.random.default_rng(n)
    E = 4 * n
    src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
    bad = rng.choice(E, 12, replace=False)
    src[bad[0:3]] = n
    dst[bad[3:6]] = n
    src[bad[6:8]] = -1
    dst[bad[8:10]] = -5
    src[bad[10]] = 2 ** 40
    dst[bad[11]] = -2 ** 40
    _check_both_builds(src.astype(np.int64), dst.astype(np.int64), n, n)


@gpu
def test_refusals_csr():
    L = _lib()
    buf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    q = _p(buf)
    ws = int(L.hscn_csr_workspace_bytes(10, 10))
    one = lambda **k: L.hscn_csr_build(*[k.get(a, d) for a, d in (
        ("key", q), ("other", q), ("E", 10), ("rows", 10), ("cols", 10), ("rowptr", q), ("col", q), ("eid", q),
        ("flag", q), ("ws", q), ("ws_bytes", ws), ("stream", _stream()))])
    for k in (dict(E=-1), dict(rows=-1), dict(rowptr=None), dict(ws=None), dict(key=None), dict(other=None),
              dict(col=None), dict(eid=None)):
        assert one(**k) == BADARG, k
    for k in (dict(E=INT32_MAX + 1), dict(rows=INT32_MAX), dict(cols=INT32_MAX + 1)):
        assert one(**k) == UNSUPPORTED, k
    assert one(ws_bytes=ws - 1) == WORKSPACE
    assert one(ws_bytes=0) == WORKSPACE
    wsp = int(L.hscn_csr_pair_workspace_bytes(10, 10, 10))
    pair = lambda **k: L.hscn_csr_build_pair(*[k.get(a, d) for a, d in (
        ("src", q), ("dst", q), ("E", 10), ("ns", 10), ("nd", 10), ("rowptr", q), ("col", q), ("eid", q),
        ("rowptr_t", q), ("col_t", q), ("eid_t", q), ("flag", q), ("ws", q), ("ws_bytes", wsp), ("stream", _stream()))])
    for k in (dict(E=-1), dict(ns=-1), dict(nd=-1), dict(rowptr=None), dict(rowptr_t=None), dict(ws=None),
              dict(src=None), dict(dst=None), dict(col=None), dict(eid=None), dict(col_t=None), dict(eid_t=None)):
        assert pair(**k) == BADARG, k
    for k in (dict(E=INT32_MAX + 1), dict(ns=INT32_MAX), dict(nd=INT32_MAX)):
        assert pair(**k) == UNSUPPORTED, k
    assert pair(ws_bytes=wsp - 1) == WORKSPACE
    assert L.hscn_csr_cross_positions(q, q, -1, q, q, _stream()) == BADARG
    for i in range(4):
        a = [q, q, q, q]
        a[i] = None
        assert L.hscn_csr_cross_positions(a[0], a[1], 5, a[2], a[3], _stream()) == BADARG
    assert L.hscn_csr_cross_positions(None, None, 0, None, None, _stream()) == 0
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0          # no refused call wrote anything


# ===================================================================================================================
# 2. Degree norms: hscn_gcn_dinv, hscn_gcn_norm_weights, hscn_gcn_norm_self_loops (csrc/structure.hip)
#
# Refusals before any launch: n < 0 (E < 0, N < 0), a NULL among the required pointers with n > 0; n == 0 (E + N == 0)
# returns 0 without a launch.                                                       [test_refusals_norms]
# k_dinv, one thread per row, blocks of 256: degree 0 -> 0 (not inf), else 1 / sqrt(d)  [n = 1, 255, 256, 257, 5000;
#                                                                                     isolated nodes in every graph]
# k_wdeg_dinv: serial float32 sum of the row's weights IN CSR ORDER (add_rn), 1 / sqrt, inf -> 0; w == NULL -> 1.0
#     degree 0 (isolated), weights that sum to 0, a zero weight, negative sums (NaN)   [weights "unit", "random", "signed"]
# k_wnorm: (dinv[col] * w) * dinv[row], two separately rounded products                [the same cases]
#   The summation order IS fixed (one thread walks its row in slot order), so the float32 reference below, which adds
#   in the same order, must agree bit for bit at every size: no float64 bound is needed here.
#   A long row                                                                        [hub of 3000 edges]
# k_gcn_norm_self_loops: launch 1 (tail = false): threads [0, E) copy the edge, weight 0 for a loop, w or 1 otherwise;
#   threads [E, E + N) write the loop of every node with `fill`; launch 2 (tail = true, only when E > 0) moves an
#   existing loop's weight to its node's tail slot, guarded by 0 <= r < N.
#     E == 0 (no second launch), N == 0, more than one block, loops present / absent,
#     both fill values (1 and 2, "improved"), weighted and unweighted, a loop on a node >= N   [test_self_loop_layout]
# ===================================================================================================================
def _norm_graph(n, E, rng, hub=0):
    src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
    iso = rng.choice(n, max(n // 10, 1), replace=False)                # nodes that receive nothing
    keep = ~np.isin(dst, iso)
    src, dst = src[keep], dst[keep]
    if hub:
        src = np.concatenate([src, rng.integers(0, n, hub)])
        dst = np.concatenate([dst, np.full(hub, (iso[0] + 1) % n)])
    return src.astype(np.int64), dst.astype(np.int64)


def _ref_norm(rowptr, col, eid, w, n):
    """Degrees summed in float32 in CSR slot order, then dis[col] * w * dis[row] with each product rounded."""
    E = int(rowptr[-1])
    wv = np.ones(E, dtype=np.float32) if w is None else w.astype(np.float32)
    d = np.diff(rowptr)
    deg = np.zeros(n, dtype=np.float32)
    for t in range(int(d.max()) if n else 0):
        rows = np.flatnonzero(d > t)
        deg[rows] = deg[rows] + wv[eid[rowptr[rows] + t]]
    with np.errstate(all="ignore"):
        r = np.float32(1.0) / np.sqrt(deg)
    dinv = np.where(np.isinf(r), np.float32(0), r).astype(np.float32)
    row_of = np.repeat(np.arange(n), d)
    wn = np.zeros(E, dtype=np.float32)
    with np.errstate(all="ignore"):
        wn[eid] = (dinv[col] * wv[eid]).astype(np.float32) * dinv[row_of]
    return dinv, wn


@gpu
@pytest.mark.parametrize("weights", ["unit", "random", "signed"])
@pytest.mark.parametrize("n,E,hub", [(1, 0, 0), (1, 3, 0), (5, 6, 0), (255, 900, 0), (256, 900, 0), (257, 900, 0),
                                     (5000, 30000, 3000)])
def test_gcn_degree_norms_bitwise(n, E, hub, weights):
    from graph_hscn import _hip
    from graph_hscn.structure import build_csr
    rng = np.random.default_rng(n + E)
    src, dst = _norm_graph(n, E, rng, hub) if n > 1 else (np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64))
    Et = src.shape[0]
    if weights == "unit":
        w = None
    elif weights == "random":
        w = rng.random(Et).astype(np.float32) * 3
        w[::7] = 0.0                                                   # zero weights
    else:
        w = rng.standard_normal(Et).astype(np.float32)                 # negative sums: NaN, as deg.pow(-0.5) gives
        if Et >= 4:
            w[1] = -w[0]
    rowptr, col, eid, _ = _ref_csr(dst, src, n, n)
    csr = build_csr(torch.from_numpy(dst).to(DEV), torch.from_numpy(src).to(DEV), n, n)
    # unweighted, from the row pointer alone
    d1 = torch.full((n,), -7.0, device=DEV)
    _hip.call("hscn_gcn_dinv", _hip.ptr(csr.rowptr), n, _hip.ptr(d1), _hip.stream())
    deg = np.diff(rowptr).astype(np.float32)
    with np.errstate(all="ignore"):
        want1 = np.where(deg > 0, np.float32(1.0) / np.sqrt(deg), np.float32(0)).astype(np.float32)
    assert np.array_equal(_bits(d1), _bits(want1))
    assert np.all(np.isfinite(d1.cpu().numpy()))
    # weighted degrees and normalised weights
    wd = None if w is None else torch.from_numpy(w).to(DEV)
    d2 = torch.full((n,), -7.0, device=DEV)
    wn = torch.full((max(Et, 1),), -7.0, device=DEV)
    _hip.call("hscn_gcn_norm_weights", _hip.ptr(csr.rowptr), _hip.ptr(csr.col), _hip.ptr(csr.eid),
              None if wd is None or Et == 0 else _hip.ptr(wd), n, _hip.ptr(d2), _hip.ptr(wn), _hip.stream())
    want_d, want_w = _ref_norm(rowptr, col, eid, None if Et == 0 else w, n)
    assert _same_floats(d2.cpu().numpy(), want_d)
    assert _same_floats(wn.cpu().numpy()[:Et], want_w)
    if w is None:
        assert np.array_equal(_bits(d2), _bits(want1))                 # unit weights: the two kernels agree
    assert not np.any(np.isinf(d2.cpu().numpy()))


@gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fill", [1.0, 2.0])
@pytest.mark.parametrize("N,E,loops", [(0, 0, 0), (1, 0, 0), (5, 0, 0), (0, 4, 0), (1, 1, 1), (5, 6, 2), (300, 1000, 0),
                                       (300, 1000, 40), (256, 256, 256), (700, 255, 9)])
def test_self_loop_layout(N, E, loops, fill, weighted):
    """hscn_gcn_norm_self_loops against its stated layout: the E edges in place (a loop keeps its slot with weight
    0), then one loop per node carrying the weight of the node's existing loop, else ``fill``."""
    from graph_hscn import _hip
    rng = np.random.default_rng(N * 3 + E + loops)
    hi = max(N, 3)
    row, col = rng.integers(0, hi, E), rng.integers(0, hi, E)
    same = row == col
    col[same] = (col[same] + 1) % hi                                   # no accidental loops
    if loops:
        at = rng.choice(E, loops, replace=False)
        nodes = rng.choice(N, loops, replace=False)                    # at most one loop per node: one winner
        row[at], col[at] = nodes, nodes
    if N == 0 and E:
        row[0] = col[0] = 2                                            # a loop on a node outside [0, N): no tail slot
    w = (rng.random(E).astype(np.float32) + 0.5) if weighted else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    r_d, c_d, w_d = dev(row.astype(np.int64)), dev(col.astype(np.int64)), dev(w)
    ro = torch.full((E + N + 1,), -9, dtype=torch.int64, device=DEV)
    co = torch.full((E + N + 1,), -9, dtype=torch.int64, device=DEV)
    wo = torch.full((E + N + 1,), -9.0, device=DEV)
    _hip.call("hscn_gcn_norm_self_loops", _hip.ptr(r_d) if E else None, _hip.ptr(c_d) if E else None,
              _hip.ptr(w_d) if (weighted and E) else None, E, N, fill, _hip.ptr(ro), _hip.ptr(co), _hip.ptr(wo),
              _hip.stream())
    wv = np.ones(E, dtype=np.float32) if w is None else w
    want_r = np.concatenate([row, np.arange(N), [-9]]).astype(np.int64)
    want_c = np.concatenate([col, np.arange(N), [-9]]).astype(np.int64)
    tail = np.full(N, fill, dtype=np.float32)
    is_loop = row == col
    inside = is_loop & (row < N)
    tail[row[inside]] = wv[inside]
    want_w = np.concatenate([np.where(is_loop, np.float32(0), wv), tail, [np.float32(-9)]]).astype(np.float32)
    assert np.array_equal(ro.cpu().numpy(), want_r) and np.array_equal(co.cpu().numpy(), want_c)
    assert np.array_equal(_bits(wo), _bits(want_w))                    # (the guard word behind the list is untouched)


@gpu
def test_refusals_norms():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    q, st = _p(buf), _stream()
    assert L.hscn_gcn_dinv(q, -1, q, st) == BADARG
    assert L.hscn_gcn_dinv(None, 3, q, st) == BADARG and L.hscn_gcn_dinv(q, 3, None, st) == BADARG
    assert L.hscn_gcn_dinv(None, 0, None, st) == 0
    assert L.hscn_gcn_norm_weights(q, q, q, None, -1, q, q, st) == BADARG
    for i in (0, 1, 2, 4, 5):
        a = [q, q, q, None, q, q]
        a[i] = None
        assert L.hscn_gcn_norm_weights(a[0], a[1], a[2], a[3], 3, a[4], a[5], st) == BADARG, i
    assert L.hscn_gcn_norm_weights(None, None, None, None, 0, None, None, st) == 0
    f = ctypes.c_float(1.0)
    assert L.hscn_gcn_norm_self_loops(q, q, None, -1, 3, f, q, q, q, st) == BADARG
    assert L.hscn_gcn_norm_self_loops(q, q, None, 3, -1, f, q, q, q, st) == BADARG
    assert L.hscn_gcn_norm_self_loops(None, q, None, 3, 3, f, q, q, q, st) == BADARG
    assert L.hscn_gcn_norm_self_loops(q, None, None, 3, 3, f, q, q, q, st) == BADARG
    for i in range(3):
        a = [q, q, q]
        a[i] = None
        assert L.hscn_gcn_norm_self_loops(q, q, None, 3, 3, f, a[0], a[1], a[2], st) == BADARG, i
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ===================================================================================================================
# 3. Dense adjacencies: hscn_to_dense_adj, _batched, _ragged, _ragged_u8 (csrc/structure.hip)
#
# Refusals before any launch: E < 0, n / B / N / nmax < 0, NULL row / col (/ adj) with E > 0, (ragged) mode outside
# {0, 1}, NULL nptr / gid / adj; E == 0 (ragged: E + (mode ? N : 0) == 0) or B == 0 returns 0 without a launch.
#                                                                                    [test_refusals_dense]
# Every kernel: one thread per edge (ragged mode 1: E + N threads, the last N add the identity), blocks of 256
#                                                                                    [E = 1 .. several thousand]
#   endpoint outside [0, N): dropped                                                  [every case adds four such edges]
#   k_dense_adj: adj[r, c] += 1, parallel edges add up                                [uniform cases, whole-batch matrix]
#   k_dense_adj_batched: r / n != c / n -> dropped (NOT written into another block)   [edges between graphs, also
#                                                                                     between the first and last graph]
#   k_dense_adj_ragged(+_u8): gid[r] != gid[c] -> dropped; mode 1 skips the list's loops and adds one per node;
#     graphs of sizes {1, nmax} in one batch; n = 1 only                              [sizes "ones", "mixed", "uniform"]
#   k_dense_adj_ragged_u8: a byte saturates at 255 through a compare-and-swap on its word: counts 254 / 255 / 256 /
#     300 in byte 0 and byte 3 of a word, the other bytes of that word and the padding columns [nmax, lda8) unchanged;
#     flag bit 16 iff some count passed 255                                           [test_byte_adjacency_saturation]
# ===================================================================================================================
def _ref_dense(row, col, sizes, nmax, mode):
    """np.add.at on a zero array; an edge must stay inside one graph, mode 1 = loops of the list out, identity in."""
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    gid = np.repeat(np.arange(len(sizes)), sizes)
    adj = np.zeros((len(sizes), nmax, nmax), dtype=np.int64)
    ok = (row >= 0) & (row < N) & (col >= 0) & (col < N)
    r, c = row[ok], col[ok]
    if mode == 1:
        nl = r != c
        r, c = r[nl], c[nl]
    same = gid[r] == gid[c]
    r, c = r[same], c[same]
    b = gid[r]
    np.add.at(adj, (b, r - ptr[b], c - ptr[b]), 1)
    if mode == 1:
        i = np.arange(N)
        np.add.at(adj, (gid, i - ptr[gid], i - ptr[gid]), 1)
    return adj


def _dense_edges(sizes, rng, per_graph=6):
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    rows, cols = [], []
    for b, n in enumerate(sizes):
        e = per_graph * n
        r, c = rng.integers(0, n, e) + ptr[b], rng.integers(0, n, e) + ptr[b]
        rows += [r, r[: e // 3], r[: e // 3]]                           # a third of the edges three times over
        cols += [c, c[: e // 3], c[: e // 3]]
    row, col = np.concatenate(rows), np.concatenate(cols)
    if len(sizes) > 1:                                                  # edges that leave their graph
        last = N - 1
        row = np.concatenate([row, [0, last, ptr[1] - 1, ptr[1]], rng.integers(0, N, 50)])
        col = np.concatenate([col, [last, 0, ptr[1], ptr[1] - 1], rng.integers(0, N, 50)])
    row = np.concatenate([row, [-1, 0, N, 0]])                          # endpoints outside the batch
    col = np.concatenate([col, [0, -1, 0, N]])
    p = rng.permutation(row.shape[0])
    return row[p].astype(np.int64), col[p].astype(np.int64), ptr, N


def _ragged(row, col, ptr, sizes, nmax, raw, as_bytes, flag=None):
    from graph_hscn.nn.pool import to_dense_adj_ragged
    ei = torch.from_numpy(np.stack([row, col])).to(DEV)
    nptr = torch.from_numpy(ptr.astype(np.int32)).to(DEV)
    gid = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)).to(DEV)
    return to_dense_adj_ragged(ei, nptr, gid, len(sizes), nmax, raw=raw, as_bytes=as_bytes, flag=flag)


@gpu
@pytest.mark.parametrize("name,sizes", [("one_node", [1]), ("ones", [1] * 5), ("uniform37", [37] * 4),
                                        ("uniform2", [2] * 300), ("mixed", [1, 40, 1, 17, 40, 1]), ("single", [130])])
def test_dense_adjacency_entry_points_agree_with_numpy(name, sizes):
    from graph_hscn.nn.pool import to_dense_adj, to_dense_adj_batched
    rng = np.random.default_rng(len(sizes) * 100 + sizes[0])
    row, col, ptr, N = _dense_edges(sizes, rng)
    nmax, B = max(sizes), len(sizes)
    for mode in (0, 1):
        want = _ref_dense(row, col, sizes, nmax, mode)
        got = _ragged(row, col, ptr, sizes, nmax, bool(mode), False)
        assert np.array_equal(_bits(got), _bits(want.astype(np.float32))), mode
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got8 = _ragged(row, col, ptr, sizes, nmax, bool(mode), True, flag)
        lda = (nmax + 31) // 32 * 32
        want8 = np.zeros((B, nmax, lda), dtype=np.uint8)
        want8[:, :, :nmax] = np.minimum(want, 255)
        assert np.array_equal(got8.cpu().numpy(), want8), mode
        assert int(flag.item()) == (16 if want.max() > 255 else 0)
    ei = torch.from_numpy(np.stack([row, col])).to(DEV)
    # the whole batch as ONE graph: edges between graphs stay, edges outside [0, N) go
    whole = _ref_dense(row, col, [N], N, 0)[0]
    assert np.array_equal(_bits(to_dense_adj(ei, N)[0]), _bits(whole.astype(np.float32)))
    if len(set(sizes)) == 1:
        got = to_dense_adj_batched(ei, B, sizes[0])
        assert np.array_equal(_bits(got), _bits(_ref_dense(row, col, sizes, nmax, 0).astype(np.float32)))


@gpu
@pytest.mark.parametrize("top", [255, 256])
def test_byte_adjacency_saturation(top):
    """Counts 254 / 255 / top / (300 when top = 256) in byte 0 and byte 3 of their words: the byte stops at 255, its
    neighbours in the word keep their own small counts, padding stays zero, bit 16 is raised iff a count passed 255."""
    sizes = [1, 12, 9]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    counts = {(1, 2, 0): 254, (1, 2, 3): 255, (1, 5, 4): top, (1, 5, 7): 254, (1, 11, 8): 300 if top == 256 else 255,
              (1, 11, 11): top, (1, 2, 1): 1, (1, 2, 2): 2, (1, 5, 5): 3, (1, 5, 6): 0, (1, 11, 9): 1, (1, 11, 10): 2,
              (2, 8, 3): top, (2, 8, 4): 255, (2, 8, 2): 5, (2, 0, 0): 254, (0, 0, 0): top}
    rows, cols = [], []
    for (b, r, c), k in counts.items():
        rows += [ptr[b] + r] * k
        cols += [ptr[b] + c] * k
    rng = np.random.default_rng(top)
    p = rng.permutation(len(rows))
    row, col = np.asarray(rows, dtype=np.int64)[p], np.asarray(cols, dtype=np.int64)[p]
    want = _ref_dense(row, col, sizes, 12, 0)
    assert want.max() == (300 if top == 256 else 255)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got8 = _ragged(row, col, ptr, sizes, 12, False, True, flag).cpu().numpy()
    want8 = np.zeros((3, 12, 32), dtype=np.uint8)
    want8[:, :, :12] = np.minimum(want, 255)
    assert np.array_equal(got8, want8)
    assert int(flag.item()) == (16 if top == 256 else 0)
    got = _ragged(row, col, ptr, sizes, 12, False, False)
    assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))     # the float form counts on


@gpu
def test_refusals_dense():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    q, st = _p(buf), _stream()
    assert L.hscn_to_dense_adj(q, q, -1, 2, q, st) == BADARG and L.hscn_to_dense_adj(q, q, 2, -1, q, st) == BADARG
    for a in ((None, q, q), (q, None, q), (q, q, None)):
        assert L.hscn_to_dense_adj(a[0], a[1], 2, 2, a[2], st) == BADARG
        assert L.hscn_to_dense_adj_batched(a[0], a[1], 2, 1, 2, a[2], st) == BADARG
    assert L.hscn_to_dense_adj(None, None, 0, 2, None, st) == 0
    for E, B, n in ((-1, 1, 2), (2, -1, 2), (2, 1, -1)):
        assert L.hscn_to_dense_adj_batched(q, q, E, B, n, q, st) == BADARG
    assert L.hscn_to_dense_adj_batched(q, q, 2, 0, 2, q, st) == 0
    for fn, extra in ((L.hscn_to_dense_adj_ragged, ()), (L.hscn_to_dense_adj_ragged_u8, (q,))):
        call = lambda row=q, col=q, E=2, nptr=q, gid=q, N=2, B=1, nmax=2, mode=0, adj=q: fn(
            row, col, E, nptr, gid, N, B, nmax, mode, adj, *extra, st)
        for k in (dict(E=-1), dict(N=-1), dict(B=-1), dict(nmax=-1), dict(mode=2), dict(mode=-1), dict(row=None),
                  dict(col=None), dict(nptr=None), dict(gid=None), dict(adj=None)):
            assert call(**k) == BADARG, k
        assert call(B=0) == 0 and call(E=0, row=None, col=None) == 0
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ===================================================================================================================
# 4. hscn_assign_argmax (csrc/structure.hip: k_argmax)
#
# Refusals before the launch: n < 0, K < 1, NULL S / ids with n > 0; n == 0 returns 0.   [test_refusals_argmax]
# One thread per row, blocks of 256                                                   [rows 1, 255, 256, 257, 300001]
# best = r[0]; the loop over k = 1 .. K-1 does not run for K == 1                     [K = 1]
# any K >= 1 (no vector path, no width limit)                                         [K = 2, 3, 5, 17, 63, 64, 65, 128, 256]
# `v > best`: the FIRST maximum wins                                                  [all-equal rows, repeated maxima,
#                                                                                     -0.0 against +0.0 (equal: first wins)]
# +-inf compare like numbers                                                          [+inf twice, all -inf, -inf then finite]
# NaN: Tensor.max(1)[1] treats a NaN as the maximum and returns the FIRST one; `v > best` alone never selects a
#   NaN after column 0, so the kernel also takes `v` when it is a NaN and `best` is not  [NaN first, last, after +inf,
#                                                                                     two NaNs, all NaN, NaN then +inf]
# ===================================================================================================================
def _argmax_rows(K, rng):
    """Rows of special values for width K (as many as fit)."""
    nan, inf = float("nan"), float("inf")
    rows = [np.zeros(K), np.full(K, -3.5), np.full(K, inf), np.full(K, -inf), np.full(K, nan)]
    z = np.zeros(K)
    z[::2] = -0.0
    rows.append(z.copy())                      # -0.0, +0.0, -0.0, ...: all equal, column 0 wins
    rows.append(-z)                            # +0.0, -0.0, ...
    for pos in sorted({0, K // 2, K - 1}):
        r = rng.standard_normal(K)
        r[pos] = nan
        rows.append(r)                         # one NaN among numbers
        r = rng.standard_normal(K)
        r[pos] = inf
        rows.append(r)
        r = np.full(K, -inf)
        r[pos] = -1e30
        rows.append(r)                         # -inf everywhere but one finite value
    if K >= 3:
        r = rng.standard_normal(K)
        r[K - 2], r[K - 1] = nan, nan
        rows.append(r)                         # two NaNs: the first one
        r = rng.standard_normal(K)
        r[0], r[K - 1] = inf, nan
        rows.append(r)                         # +inf then NaN: the NaN
        r = rng.standard_normal(K)
        r[1], r[K - 1] = nan, inf
        rows.append(r)                         # NaN then +inf: the NaN
        r = rng.standard_normal(K)
        r[1], r[K - 1] = inf, inf
        rows.append(r)                         # +inf twice: the first
        r = np.full(K, 2.0)
        r[0] = 1.0
        rows.append(r)                         # the maximum repeated from column 1 on
    return np.stack(rows).astype(np.float32)


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 300001])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 17, 63, 64, 65, 128, 256])
def test_argmax_equals_tensor_max(K, n):
    from graph_hscn import _hip
    if n * K > 8_000_000:
        n = 8_000_000 // K                     # (32 MB; still 31250 rows at K = 256, 122 blocks of 256 threads)
    rng = np.random.default_rng(K * 1000 + n % 1000)
    S = torch.softmax(torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)) * 30, -1)  # saturating: exact ties
    S[::7] = S[::7].round()
    special = torch.from_numpy(_argmax_rows(K, rng))
    m = min(special.size(0), n)
    S[n - m:] = special[:m]                    # in the LAST rows: the last block of the grid
    if n > 2 * m:
        S[:m] = special[:m]
    ids = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    Sd = S.to(DEV)
    _hip.call("hscn_assign_argmax", _hip.ptr(Sd), _hip.ptr(ids), n, K, _hip.stream())
    want = S.max(1)[1].numpy()
    got = ids.cpu().numpy()
    assert np.array_equal(got[:n], want)
    assert got[n] == -7


def test_tensor_max_rule_the_argmax_kernel_follows():
    """The reference's rule itself (train_clustering.py:68 uses Tensor.max(1)[1]): first maximum, first NaN."""
    nan, inf = float("nan"), float("inf")
    S = torch.tensor([[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, 0.0, -0.0], [1.0, nan, 5.0, nan], [inf, 1.0, nan, inf],
                      [nan, nan, nan, nan], [-inf, -inf, -inf, -inf]])
    assert S.max(1)[1].tolist() == [1, 0, 1, 2, 0, 0]


@gpu
def test_refusals_argmax():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    q, st = _p(buf), _stream()
    assert L.hscn_assign_argmax(q, q, -1, 4, st) == BADARG
    assert L.hscn_assign_argmax(q, q, 4, 0, st) == BADARG and L.hscn_assign_argmax(q, q, 4, -2, st) == BADARG
    assert L.hscn_assign_argmax(None, q, 4, 4, st) == BADARG and L.hscn_assign_argmax(q, None, 4, 4, st) == BADARG
    assert L.hscn_assign_argmax(None, None, 0, 4, st) == 0
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ===================================================================================================================
# 5. Hetero build: hscn_build_hetero_count / _scan / _emit (csrc/hetero_build.hip)
#
# Refusals before any launch: count: B < 1, F < 1, K < 1, K > 64 (HB_KMAX) -> BADARG, F > 16 (HB_FMAX) -> UNSUPPORTED,
# a NULL array -> BADARG; scan: B < 1, NULL; emit: B < 1, F < 1, K < 1, K > 64, N < 0, Evv < 0, NULL.
#                                                                                    [test_refusals_hetero_build]
# k_hetero_count, one workgroup of 256 per graph:
#   node loops stride 256                                                            [n = 1, 127 .. 129, 255 .. 257, 300, 384]
#   64-bit presence mask, 1 << c with c up to 63; remap[k] = popcount below k         [K = 63 / 64 with ids 62 and 63 in use;
#                                                                                     one id only (U = 1); every id (U = K);
#                                                                                     an id used by the last node alone]
#   an id outside [0, K): flag |= 8 (-> IndexError)                                   [test_hetero_build_bad_ids, graph 300]
#   float64 sums in node order over staged chunks of HB_CH = 128 nodes                [n = 127, 128, 129, 256, 384 (3 chunks)]
#   one thread per (virtual slot, feature) pair, HB_VFPT = 4 pairs per thread         [U F = 1 (K = 1, F = 1) .. 1024
#                                                                                     (U = 64, F = 16)]
#   virtual v <- remapped cluster (v + 1) mod U                                       [U = 1: (0 + 1) mod 1 = 0]
#   x as float32 or int64 (two instantiations)                                       [dtype float32 / int64]
# k_hetero_scan, ONE workgroup, graphs 256 per trip with a carry (vptr, evptr, max U)   [B = 1, 255, 256, 257, 600]
# k_hetero_emit, one workgroup per graph: loops stride 256 over U F, U, n and the vv blocks   [the same cases]
# ===================================================================================================================
def _hetero_case(ns, ids, F, K, dtype, rng):
    """Data graphs with n nodes and the given cluster ids; features are random floats (float32 case: the order of the
    float64 sum matters) or small integers (int64 case)."""
    from graph_hscn.data import Data
    graphs = []
    for n in ns:
        if dtype == torch.int64:
            x = torch.from_numpy(rng.integers(0, 30, (n, F)))
        else:
            x = torch.from_numpy((rng.standard_normal((n, F)) * 10).astype(np.float32))
        e = rng.integers(0, n, (2, 2 * n))
        graphs.append(Data(x=x, edge_index=torch.from_numpy(e.astype(np.int64)), y=torch.zeros(1, 3)))
    return graphs, [np.asarray(i, dtype=np.int64) for i in ids]


def _check_hetero(graphs, ids, K, oracle):
    from graph_hscn.data import Batch, HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_batch_on_device, hetero_from_clusters
    host = HeteroBatch.from_data_list([hetero_from_clusters(g, i, K) for g, i in zip(graphs, ids)])
    big = Batch.from_data_list(graphs).to(DEV)
    hb = hetero_batch_on_device(big, torch.from_numpy(np.concatenate(ids)).to(DEV), K)
    assert np.array_equal(_bits(hb["virtual"].x), _bits(host["virtual"].x))       # float32 casts of float64 means
    assert np.array_equal(_bits(hb["local"].x), _bits(host["local"].x.float()))
    for et in (LL, VV, LV):
        assert torch.equal(hb[et].edge_index.cpu(), host[et].edge_index), et
        assert torch.equal(hb[et].ptr32.cpu(), host[et].ptr32), et
    for nt in ("local", "virtual"):
        assert torch.equal(hb[nt].batch.cpu(), host[nt].batch)
        assert torch.equal(hb[nt].ptr.cpu(), host[nt].ptr) and torch.equal(hb[nt].ptr32.cpu(), host[nt].ptr32)
        assert hb[nt].max_nodes == host[nt].max_nodes and hb[nt].num_nodes == host[nt].num_nodes
    assert hb[VV].max_edges == host[VV].max_edges
    if oracle:
        from oracle import hetero_data as OH
        want = OH.collate_hetero([OH.hetero_from_clusters(g.x, g.edge_index, g.y, i, K) for g, i in zip(graphs, ids)])
        assert np.array_equal(_bits(hb["virtual"].x), _bits(want["x_dict"]["virtual"]))
        for et, key in ((LL, OH.LL), (VV, OH.VV), (LV, OH.LV)):
            assert torch.equal(hb[et].edge_index.cpu(), want["edge_index_dict"][key])
        assert torch.equal(hb["virtual"].batch.cpu(), want["batch_virtual"])


def _id_pattern(kind, n, K, rng):
    if kind == "random":
        return rng.integers(0, K, n)
    if kind == "one_id":                       # U = 1
        return np.full(n, K - 1)
    if kind == "every_id":                     # U = min(n, K) = K when n >= K
        return np.concatenate([np.arange(K), rng.integers(0, K, max(n - K, 0))])[:n]
    if kind == "top_two":                      # only the two highest ids: bits K-2 and K-1 of the mask
        return rng.integers(K - 2, K, n) if K >= 2 else np.zeros(n, dtype=np.int64)
    if kind == "last_node":                    # the highest id appears at the last node only
        i = rng.integers(0, max(K - 1, 1), n)
        i[-1] = K - 1
        return i
    raise KeyError(kind)


_HETERO_EDGES = [(n, F, K, kind, dt)
                 for n, F, K, kind, dt in
                 [(1, 1, 1, "one_id", torch.float32), (1, 16, 64, "one_id", torch.float32),
                  (127, 9, 16, "random", torch.float32), (128, 9, 16, "random", torch.float32),
                  (129, 9, 16, "random", torch.float32), (129, 9, 16, "last_node", torch.int64),
                  (255, 3, 5, "random", torch.int64), (256, 3, 5, "random", torch.float32),
                  (257, 3, 5, "last_node", torch.float32), (384, 14, 64, "random", torch.float32),
                  (300, 16, 64, "every_id", torch.float32), (300, 16, 64, "every_id", torch.int64),
                  (300, 16, 63, "every_id", torch.float32), (200, 16, 64, "top_two", torch.float32),
                  (200, 2, 63, "top_two", torch.int64), (130, 1, 64, "last_node", torch.int64),
                  (130, 1, 7, "random", torch.int64), (70, 16, 64, "one_id", torch.float32),
                  (40, 16, 64, "every_id", torch.float32)]]


@gpu
@pytest.mark.parametrize("n,F,K,kind,dtype", _HETERO_EDGES)
def test_hetero_build_at_chunk_mask_and_width_edges(n, F, K, kind, dtype):
    """Three graphs per case: the edge graph between a 1-node graph and a mid-size one, so that offsets matter.
    F = 1 compares with the oracle only on integer features (any summation order is exact there)."""
    rng = np.random.default_rng(n * 131 + F * 7 + K)
    ns = [1, n, 33]
    ids = [_id_pattern("one_id", 1, K, rng), _id_pattern(kind, n, K, rng), _id_pattern("random", 33, K, rng)]
    graphs, ids = _hetero_case(ns, ids, F, K, dtype, rng)
    _check_hetero(graphs, ids, K, oracle=n <= 300 and (F > 1 or dtype == torch.int64))


@gpu
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_hetero_build_scan_carries_between_trips(B):
    """k_hetero_scan walks 256 graphs per trip: the per-graph cluster counts vary, so a lost carry moves every offset
    of the graphs past 256."""
    rng = np.random.default_rng(B)
    K, F = 7, 3
    ns = [int(v) for v in rng.integers(1, 13, B)]
    ids = [_id_pattern(["random", "one_id", "last_node"][j % 3], n, K, rng) for j, n in enumerate(ns)]
    graphs, ids = _hetero_case(ns, ids, F, K, torch.float32, rng)
    _check_hetero(graphs, ids, K, oracle=B <= 257)


@gpu
def test_hetero_build_bad_ids_past_the_first_scan_trip():
    from graph_hscn.data import Batch
    from graph_hscn.loader.hetero_data import hetero_batch_on_device
    rng = np.random.default_rng(5)
    ns = [3] * 400
    graphs, ids = _hetero_case(ns, [rng.integers(0, 4, 3) for _ in ns], 2, 4, torch.float32, rng)
    big = Batch.from_data_list(graphs).to(DEV)
    for bad in (4, -1):
        flat = np.concatenate(ids)
        flat[3 * 300 + 1] = bad
        with pytest.raises(IndexError):
            hetero_batch_on_device(big, torch.from_numpy(flat).to(DEV), 4)


@gpu
def test_refusals_hetero_build():
    L = _lib()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    q, st = _p(buf), _stream()
    count = lambda x=q, i64=0, cl=q, nptr=q, B=1, F=2, K=4, U=q, lvl=q, means=q: L.hscn_build_hetero_count(
        x, i64, cl, nptr, B, F, K, U, lvl, means, q, st)
    for k in (dict(B=0), dict(B=-1), dict(F=0), dict(K=0), dict(K=65), dict(x=None), dict(cl=None), dict(nptr=None),
              dict(U=None), dict(lvl=None), dict(means=None)):
        assert count(**k) == BADARG, k
    assert count(F=17) == UNSUPPORTED and count(F=17, i64=1) == UNSUPPORTED
    assert L.hscn_build_hetero_scan(q, 0, q, q, q, q, q, q, st) == BADARG
    for i in (0, 2, 3, 4, 5, 6):
        a = [q] * 7
        a[i] = None
        assert L.hscn_build_hetero_scan(a[0], 1, a[1], a[2], a[3], a[4], a[5], a[6], st) == BADARG, i
    emit = lambda U=q, vptr=q, evptr=q, nptr=q, lvl=q, means=q, B=1, F=2, K=4, N=1, Evv=1, vx=q, lv=q, vv=q: \
        L.hscn_build_hetero_emit(U, vptr, evptr, nptr, lvl, means, B, F, K, N, Evv, vx, lv, vv, q, st)
    for k in (dict(B=0), dict(F=0), dict(K=0), dict(K=65), dict(N=-1), dict(Evv=-1), dict(U=None), dict(vptr=None),
              dict(evptr=None), dict(nptr=None), dict(lvl=None), dict(means=None), dict(vx=None), dict(lv=None),
              dict(vv=None)):
        assert emit(**k) == BADARG, k
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0


# ===================================================================================================================
# 6. Device collate: hscn_collate_gather, hscn_collate_gather_structure (csrc/collate.hip)
#
# Refusals before any launch: NULL ds / out (/ dss / outs), B < 0, B > 65535 -> BADARG; B == 0 returns 0; then NULL
# ids or a NULL / non-positive field of the structs -> BADARG.                        [test_refusals_collate]
# grid (B, 6) / (B, 4), one block of 256 per (slot j, part):
#   slot_ranges: the sizes of the j ids before slot j, 256 per trip: blocks with j > 256 take a second trip,
#     j > 512 a third                                                                 [B = 255, 256, 257, 600]
#   an id outside [0, G): flag |= 8, the block writes nothing                         [ids G, -1 and 2^40 in slots 300 / 2 /
#                                                                                     599 of B = 600]
#     slot_ranges of the LATER slots skips such an id (`g < 0 || g >= G`): before these cases existed it read the
#     range tables through it, out of bounds -- the old 3-slot test only ever read one entry past the end
#   a range that does not fit the static capacity: flag |= 8                          [B copies of the largest graph]
#   copy loops stride 256 over n F, n, nv F, nv, edges; part 5 writes the tables, slot B - 1 the totals
#     a 1-node / 0-edge graph (empty ll range), first and last graph of the dataset,
#     repeated ids                                                                    [graph 0 is that graph; ids hold 0 and
#                                                                                     G - 1, and 0 many times]
#   cursor != NULL: ids += cursor * B, then k_cursor_advance                          [test_collate_cursor_walk: two epochs,
#                                                                                     one replay past the epoch's end (the
#                                                                                     spare batch of valid ids), the rewind]
#   hscn_collate_gather_structure: the same slot_ranges over two tables, CSR slices copied as they are   [B = 257]
# ===================================================================================================================
def _collate_dataset(G, seed, K=4, F=9):
    """Small synthetic hetero graphs; graph 0 has one node and no edge, the last one is the largest."""
    from graph_hscn.data import Data
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    rng = np.random.default_rng(seed)
    hs = []
    for g in range(G):
        n = 1 if g == 0 else (14 if g == G - 1 else int(rng.integers(1, 12)))
        e = 0 if g == 0 else int(rng.integers(0, 3 * n + 1))
        ei = torch.from_numpy(rng.integers(0, n, (2, e)).astype(np.int64))
        x = torch.from_numpy(rng.integers(0, 20, (n, F)))
        y = torch.from_numpy((rng.random((1, 5)) < 0.4).astype(np.float32))
        hs.append(hetero_from_clusters(Data(x=x, edge_index=ei, y=y), rng.integers(0, K, n), K))
    return hs


def _same_batch(static_hb, host):
    for nt in ("local", "virtual"):
        n = host[nt].num_nodes
        assert np.array_equal(_bits(static_hb[nt].x[:n]), _bits(host[nt].x.float()))
        assert torch.equal(static_hb[nt].batch[:n].cpu(), host[nt].batch)
        assert torch.equal(static_hb[nt].ptr.cpu(), host[nt].ptr) and torch.equal(static_hb[nt].ptr32.cpu(), host[nt].ptr32)
    assert np.array_equal(_bits(static_hb["local"].y), _bits(host["local"].y.float()))
    for et in (LL, VV, LV):
        e = host[et].edge_index.size(1)
        assert torch.equal(static_hb[et].edge_index[:, :e].cpu(), host[et].edge_index), et
        assert torch.equal(static_hb[et].ptr32.cpu(), host[et].ptr32), et


@gpu
@pytest.mark.parametrize("B", [255, 256, 257, 600])
def test_collate_gather_past_one_trip_of_slots(B):
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.device_dataset import DeviceHeteroDataset
    G = B + 5
    hs = _collate_dataset(G, seed=B)
    ds = DeviceHeteroDataset(hs, DEV, B)
    rng = np.random.default_rng(B)
    plain = rng.permutation(G)[:B]
    inner = rng.permutation(np.arange(1, G - 1))[: B - 2]
    ends = np.concatenate([inner, [G - 1, 0]])           # first and last graph of the dataset, in the last slots
    repeated = plain.copy()                              # the smallest graph (smallest in every table) in a third of
    repeated[rng.choice(B, B // 3, replace=False)] = 0   # the slots: within the capacity of B distinct graphs
    repeated[B - 1] = repeated[B - 2] = 3                # and another graph twice, in the last trip
    largest = np.argsort([-h["local"].num_nodes for h in hs], kind="stable")[:B]
    for ids in (plain, ends, repeated, largest):
        hb = ds.gather(torch.as_tensor(ids, dtype=torch.int64, device=DEV))
        ds.check()
        _same_batch(hb, HeteroBatch.from_data_list([hs[i] for i in ids]))


@gpu
def test_collate_flags_bad_ids_and_overflow_past_the_first_trip():
    from graph_hscn.loader.device_dataset import DeviceHeteroDataset
    B, G = 600, 605
    hs = _collate_dataset(G, seed=1)
    good = np.random.default_rng(0).permutation(G)[:B]
    for slot, bad in ((300, G), (2, -1), (599, 2 ** 40)):
        ds = DeviceHeteroDataset(hs, DEV, B)
        ids = good.copy()
        ids[slot] = bad
        ds.gather(torch.as_tensor(ids, dtype=torch.int64, device=DEV))
        with pytest.raises(IndexError):
            ds.check()
    ds = DeviceHeteroDataset(hs, DEV, B)
    ds.gather(torch.as_tensor(good, dtype=torch.int64, device=DEV))
    ds.check()
    ds.gather(torch.full((B,), G - 1, dtype=torch.int64, device=DEV))       # B copies of the largest graph do not fit
    with pytest.raises(IndexError):
        ds.check()


@gpu
def test_collate_structure_gather_past_one_trip_of_slots():
    from graph_hscn.data import HeteroBatch
    from graph_hscn.engine import build_structure
    from graph_hscn.loader.device_dataset import DeviceHeteroDataset
    B, G = 257, 262
    hs = _collate_dataset(G, seed=9)
    ds = DeviceHeteroDataset(hs, DEV, B, resident_structure=True)
    ids = np.random.default_rng(3).permutation(G)[:B]
    ids[B - 1] = 0
    hb = ds.gather(torch.as_tensor(ids, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    ds.check()
    host = HeteroBatch.from_data_list([hs[i] for i in ids])
    _same_batch(hb, host)
    ref = build_structure(host.to(DEV))
    torch.cuda.synchronize()
    for k, v in ref.t.items():
        if v.numel() > 1:
            a, b = hb.structure.t[k][: v.numel()], v
            if a.dtype == torch.float32:
                assert np.array_equal(_bits(a), _bits(b)), k
            else:
                assert torch.equal(a, b), k


@gpu
def test_collate_cursor_walk_across_the_end_of_an_epoch():
    """gather_next: batch number `cursor` of the device-resident permutation.  Two epochs of G // B batches; one
    more replay than the epoch holds reads the permutation's tail and the spare batch of valid ids behind it; a new
    epoch rewinds the counter."""
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.device_dataset import DeviceHeteroDataset
    B, G = 257, 600
    hs = _collate_dataset(G, seed=2)
    ds = DeviceHeteroDataset(hs, DEV, B)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for epoch in range(2):
        perm = ds.new_epoch(gen).clone().cpu().numpy()
        assert int(ds._cursor.item()) == 0
        for i in range(G // B):
            hb = ds.gather_next()
            _same_batch(hb, HeteroBatch.from_data_list([hs[j] for j in perm[i * B:(i + 1) * B]]))
            assert int(ds._cursor.item()) == i + 1
        ds.check()
    assert sorted(perm.tolist()) == list(range(G))
    buf = ds._perm_buf.cpu().numpy()
    tail = buf[2 * B: 3 * B]                               # 86 ids of the permutation, then graph 0 from the spare
    assert tail.shape[0] == B and np.all(tail[G - 2 * B:] == 0)
    hb = ds.gather_next()
    ds.check()
    _same_batch(hb, HeteroBatch.from_data_list([hs[j] for j in tail]))
    perm = ds.new_epoch(gen).clone().cpu().numpy()
    hb = ds.gather_next()
    _same_batch(hb, HeteroBatch.from_data_list([hs[j] for j in perm[:B]]))
    ds.check()


@gpu
def test_refusals_collate():
    from graph_hscn.loader.device_dataset import DeviceHeteroDataset
    L = _lib()
    ds = DeviceHeteroDataset(_collate_dataset(8, seed=4), DEV, 4, resident_structure=True)
    ids = torch.arange(4, dtype=torch.int64, device=DEV)
    hb = ds.gather(ids)
    torch.cuda.synchronize()
    before = {nt: hb[nt].x.clone() for nt in ("local", "virtual")}
    d, o, s, t = (ctypes.byref(v) for v in (ds._ds, ds._out, ds.structure.c, ds._out_structure.c))
    q, fl, st = _p(ids), _p(ds.flag), _stream()
    assert L.hscn_collate_gather(None, q, 4, o, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather(d, q, 4, None, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather(d, q, -1, o, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather(d, q, 65536, o, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather(d, None, 4, o, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather(d, None, 0, o, fl, None, None, st) == 0
    for a in ((None, s, o, t), (d, None, o, t), (d, s, None, t), (d, s, o, None)):
        assert L.hscn_collate_gather_structure(a[0], a[1], q, 4, a[2], a[3], fl, None, None, st) == BADARG
    assert L.hscn_collate_gather_structure(d, s, q, -1, o, t, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather_structure(d, s, q, 65536, o, t, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather_structure(d, s, None, 4, o, t, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather_structure(d, s, None, 0, o, t, fl, None, None, st) == 0
    # a struct with a missing field
    broken = type(ds._ds).from_buffer_copy(ds._ds)
    broken.F = 0
    assert L.hscn_collate_gather(ctypes.byref(broken), q, 4, o, fl, None, None, st) == BADARG
    broken = type(ds._ds).from_buffer_copy(ds._ds)
    broken.G = 0
    assert L.hscn_collate_gather(ctypes.byref(broken), q, 4, o, fl, None, None, st) == BADARG
    assert L.hscn_collate_gather_structure(ctypes.byref(broken), s, q, 4, o, t, fl, None, None, st) == BADARG
    torch.cuda.synchronize()
    ds.check()
    for nt in ("local", "virtual"):
        assert torch.equal(hb[nt].x, before[nt])


# ===================================================================================================================
# 7. Dropout: hscn_dropout (csrc/dropout.hip) and the same generator inside k_mpnn_step (csrc/resident_mpnn.hip,
#    csrc/hscn_common.h: philox4x32_10, dropout_keep_rule)
#
# Refusals before the launch: count < 0, p outside [0, 1) (p = 1, p < 0, NaN), NULL x / y with count > 0; count == 0
# returns 0.                                                                          [test_refusals_dropout]
# Generator: Philox-4x32-10, counter (quad index low, high, 0, 0), key (seed low, seed high)   [the reference below is
#                                                                                     pinned to the published vectors
#                                                                                     on the CPU; seeds with a high half]
# threshold = floor(p 2^32), saturating at 2^32 - 1 (out of reach of a float32 p < 1: the largest, 1 - 2^-24, gives
#   2^32 - 256); scale = 1 / (1 - p) in float32                                        [p = 0, 0.2, 0.5, 1 - 2^-24]
# k_dropout: one thread per quad, grid capped at 4096 blocks of 256 -> a grid-stride second trip past 4 194 304
#   elements                                                                          [count 4 194 304 + 5]
#   full quad with x and y both 16-byte aligned: float4 path; otherwise the scalar loop, which also ends the
#   partial last quad                                                                 [counts 1 .. 5, 1023; x, y or both
#                                                                                     off by one float]
# k_mpnn_step: element (row, o) of hidden layer l at step t draws word (gi & 3) of quad gi >> 2, gi = row H + o with
#   the batch-global row, key seed0 + (L - 1) t + l                                    [test_mpnn_step_keeps_what_philox_says]
# ===================================================================================================================
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox-4x32-10 (Salmon et al., Random123): ``ctr`` uint64 array [n, 4] of 32-bit words, ``key`` two 32-bit
    words -> uint32 [n, 4]."""
    c0, c1, c2, c3 = (np.asarray(ctr, dtype=np.uint64)[:, i].copy() for i in range(4))
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    mask = np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 -> 64 bits: no overflow
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def dropout_draws(count, seed):
    """The draw of each of ``count`` elements: word i % 4 of block i // 4 under key ``seed``."""
    quads = np.arange((count + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((quads.shape[0], 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = quads & np.uint64(_MASK), quads >> np.uint64(32)
    return philox4x32_10(ctr, (seed & _MASK, (seed >> 32) & _MASK)).reshape(-1)[:count]


def keep_mask(count, p, seed):
    p32 = float(np.float32(p))
    return dropout_draws(count, seed).astype(np.uint64) >= np.uint64(int(np.floor(p32 * 2.0 ** 32)))


def test_philox_reference_known_answers():
    """The three published known-answer vectors of Philox-4x32-10 (Random123 kat_vectors)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((_MASK,) * 4, (_MASK, _MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.asarray([ctr], dtype=np.uint64), key)[0]
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]
    # all three at once through the vector path, one key at a time
    both = philox4x32_10(np.asarray([kat[0][0], kat[0][0]], dtype=np.uint64), kat[0][1])
    assert np.array_equal(both[0], both[1])
    # the element numbering of dropout_draws: quad q holds elements 4 q .. 4 q + 3
    d = dropout_draws(7, 0)
    assert [int(v) for v in d[:4]] == list(kat[0][2])
    assert [int(v) for v in dropout_draws(4, (0xFFFFFFFF << 32) | 0xFFFFFFFF)] != list(kat[1][2])   # (counter 0, not ~0)


_SEEDS = [7, 0x9E3779B97F4A7C15, (0xDEADBEEF << 32) | 1]


@gpu
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5, 1.0 - 2.0 ** -24])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 1023, 4194304 + 5])
def test_dropout_equals_the_philox_reference(count, p):
    """Through the C call (p = 0 included): y = x * scale where the reference keeps, 0 elsewhere, bit for bit, for
    aligned and misaligned x / y and every seed."""
    from graph_hscn import _hip
    rng = np.random.default_rng(count % 1000)
    x_np = (rng.standard_normal(count) * 4).astype(np.float32)
    x_np[x_np == 0] = 1.0
    p32 = np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    bases = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 3)] if count < 10000 else [(0, 0), (1, 1)]
    seeds = _SEEDS if count < 10000 else _SEEDS[1:2]
    for seed in seeds:
        keep = keep_mask(count, p, seed)
        want = np.where(keep, (x_np * scale).astype(np.float32), np.float32(0))
        for ox, oy in bases:
            xb = torch.zeros(count + 8, device=DEV)
            yb = torch.full((count + 8,), -7.0, device=DEV)
            x, y = xb[ox: ox + count], yb[oy: oy + count]
            x.copy_(torch.from_numpy(x_np))
            _hip.call("hscn_dropout", _hip.ptr(x), _hip.ptr(y), count, float(p32), seed, _hip.stream())
            got = yb.cpu().numpy()
            assert np.array_equal(_bits(got[oy: oy + count]), _bits(want)), (seed, ox, oy)
            assert np.all(got[:oy] == -7.0) and np.all(got[oy + count:] == -7.0)       # nothing outside [0, count)
        if p == 0.0:
            assert keep.all()
        if count > 10000 and 0 < p < 0.9:
            assert abs(float(keep.mean()) - (1 - p)) < 0.01        # (sanity of the reference itself, not of the kernel)


@gpu
@pytest.mark.parametrize("p", [0.2, 0.5, 1.0 - 2.0 ** -24])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 1023, 4194304 + 5])
def test_functional_dropout_mask_equals_the_philox_reference(count, p):
    """nn.functional.dropout(ones, p, True, seed): kept exactly where draw >= floor(p 2^32), kept values 1 / (1 - p);
    the backward regenerates the same mask."""
    from graph_hscn.nn import functional as Fh
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for seed in (_SEEDS if count < 10000 else _SEEDS[2:]):
        keep = keep_mask(count, p, seed)
        ones = torch.ones(count, device=DEV, requires_grad=True)
        y = Fh.dropout(ones, p, True, seed)
        assert np.array_equal(y.detach().cpu().numpy() != 0, keep), seed
        assert np.array_equal(_bits(y), _bits(np.where(keep, scale, np.float32(0)))), seed
        y.backward(torch.full((count,), 3.0, device=DEV))
        assert np.array_equal(_bits(ones.grad), _bits(np.where(keep, np.float32(3.0) * scale, np.float32(0)))), seed


@gpu
def test_mpnn_step_keeps_what_philox_says():
    """MPNNResidentTrainStep with seed0: graphs without neighbours (only a loop edge, which the step drops), node i of
    a graph carries 2^i in feature 0, layer 0 copies it into all H columns, the later layers are the identity, p = 0.5
    (scale 2).  Every value is a power of two and every sum is exact, so pred[g, o] = (sum_i 4 * 2^i keep0 keep1) / n
    reveals the two masks of every element: it must equal the Philox reference's, bit for bit, at steps 0 and 1
    (keys seed0 + 2 t + l)."""
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.data import Batch, Data
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.step import MPNNResidentTrainStep
    F, H, C, Lyr, p = 9, 16, 16, 3, 0.5
    seed0 = (0x1234ABCD << 32) | 0x00C0FFEE
    rng = np.random.default_rng(0)
    ns = [1, 2, 3, 20, 1, 7, 16, 5, 1, 11] * 4
    graphs = []
    for n in ns:
        x = rng.integers(-5, 6, (n, F)).astype(np.float32)
        x[:, 0] = 2.0 ** np.arange(n)
        graphs.append(Data(x=torch.from_numpy(x), edge_index=torch.zeros(2, 1, dtype=torch.int64), y=torch.zeros(1, C)))
    b = Batch.from_data_list(graphs)
    pm = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], F, H, C, Lyr, p).to(DEV)
    with torch.no_grad():
        w0 = torch.zeros(H, F)
        w0[:, 0] = 1.0
        for i, c in enumerate(pm.conv_layers):
            c.lin.weight.copy_(w0 if i == 0 else torch.eye(H))
            c.bias.zero_()
    pm.train()
    bd = b.to(DEV)
    bd.x = bd.x.float().contiguous()
    step = MPNNResidentTrainStep(pm, bd, "cross_entropy", seed0=seed0)
    N = sum(ns)
    ptr = np.concatenate([[0], np.cumsum(ns)])
    val = np.concatenate([2.0 ** np.arange(n) for n in ns])[:, None]            # [N, 1]
    seen = []
    for t in range(2):
        step.run()
        torch.cuda.synchronize()
        step.check()
        k0 = keep_mask(N * H, p, (seed0 + (Lyr - 1) * t) & 0xFFFFFFFFFFFFFFFF).reshape(N, H)
        k1 = keep_mask(N * H, p, (seed0 + (Lyr - 1) * t + 1) & 0xFFFFFFFFFFFFFFFF).reshape(N, H)
        a2 = (val * 4.0 * k0 * k1).astype(np.float32)                            # exact: powers of two
        want = np.stack([a2[ptr[g]:ptr[g + 1]].sum(0, dtype=np.float32) / np.float32(ns[g]) for g in range(len(ns))])
        assert np.array_equal(_bits(step.pred), _bits(want.astype(np.float32))), t
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])
    one = np.asarray(ns) == 1                              # one-node graphs: an element survives both masks 1 time in 4
    assert 0.1 < float((seen[0][one] != 0).mean()) < 0.4   # (the construction does show the masks)


@gpu
def test_refusals_dropout():
    L = _lib()
    buf = torch.zeros(64, device=DEV)
    q, st = _p(buf), _stream()
    f = ctypes.c_float
    assert L.hscn_dropout(q, q, -1, f(0.5), 1, st) == BADARG
    for p in (1.0, 1.5, -0.25, float("nan")):
        assert L.hscn_dropout(q, q, 8, f(p), 1, st) == BADARG, p
    assert L.hscn_dropout(None, q, 8, f(0.5), 1, st) == BADARG and L.hscn_dropout(q, None, 8, f(0.5), 1, st) == BADARG
    assert L.hscn_dropout(None, None, 0, f(0.5), 1, st) == 0
    torch.cuda.synchronize()
    assert float(buf.abs().sum().item()) == 0.0
