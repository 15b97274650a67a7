"""hscn_resident_launch_plan: the size-dependent choices of the graph-resident launch pair, asked from the host
(no launch, no device: runs without a GPU).  The GPU tests name the branch they exercise through this query
(tests/test_gpu_resident_f64.py); here its own consistency."""
import ctypes

import pytest

WIDTHS = [(9, 16, 3, 10), (16, 16, 1, 1), (9, 32, 2, 11), (32, 32, 3, 32), (9, 64, 2, 10), (1, 64, 1, 21)]
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 440, 444, 500, 700, 1000, 2000, 5000]


def _shapes():
    for n in SIZES:
        for ell in (0, 2 * n, 8 * n + 3, 40 * n):
            for K in (1, 8, 64):
                yield n, min(K, max(n, 1)), ell, K * (K + 1) // 2


def _plan(*a, **k):
    from graph_hscn import _hip
    return _hip.resident_launch_plan(*a, **k)


@pytest.mark.parametrize("F,H,L,C", WIDTHS)
def test_plan_agrees_with_supported(F, H, L, C):
    from graph_hscn import _hip
    lib = _hip.lib()
    seen = set()
    for n, v, ell, evv in _shapes():
        for want in (False, True):
            p = _plan(F, H, L, C, n, v, ell, evv, want)
            ok = lib.hscn_resident_supported(F, H, L, C, n, v, ell, evv) == 1
            seen.add(ok)
            assert (p is not None) == ok, (n, v, ell, evv, want)
            if p is None:
                continue
            assert set(p) == set(_hip.PLAN_FIELDS)
            assert 0 < p["fwd_lds"] <= 160 * 1024 and 0 < p["bwd_lds"] <= 160 * 1024
            assert p["db"] in (0, 1) and p["exp"] in (0, 1) and p["two"] in (0, 1) and p["csr_launch"] in (0, 1)
            # the export happens in exactly one place when it is wanted, nowhere when it is not
            assert p["exp"] + p["csr_launch"] == (1 if want else 0), (n, v, ell, evv, want, p)
    assert seen == {False, True}, "the shapes straddle the envelope"


def test_plan_refuses_what_supported_refuses():
    from graph_hscn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_int32 * len(_hip.PLAN_FIELDS))()
    assert lib.hscn_resident_launch_plan(9, 24, 3, 10, 100, 8, 200, 36, 1, buf) == -3       # H must be 16/32/64
    assert lib.hscn_resident_launch_plan(17, 16, 3, 10, 100, 8, 200, 36, 1, buf) == -3      # F <= H
    assert lib.hscn_resident_launch_plan(9, 16, 3, 10, 5000, 16, 10000, 136, 1, buf) == -3  # does not fit LDS
    assert lib.hscn_resident_launch_plan(9, 16, 3, 10, -1, 16, 100, 136, 1, buf) == -3
    assert lib.hscn_resident_launch_plan(9, 16, 3, 10, 100, 8, 200, 36, 1, None) == -1      # HSCN_E_BADARG
    assert _plan(9, 24, 3, 10, 100, 8, 200, 36) is None


@pytest.mark.parametrize("F,H,L,C", WIDTHS)
def test_256_threads_hold_exactly_up_to_64_nodes(F, H, L, C):
    for n in range(0, 100):
        p = _plan(F, H, L, C, n, min(8, max(n, 1)), 4 * n, 36)
        assert p is not None, n
        assert p["threads"] == (256 if n <= 64 else 1024), (n, p)


@pytest.mark.parametrize("F,H,L,C", WIDTHS)
@pytest.mark.parametrize("edges_per_node", [0, 2, 6])
def test_two_buffer_backward_is_monotone_in_the_graph_size(F, H, L, C, edges_per_node):
    """Once the three n x H buffers no longer fit they never fit again at a larger graph: ``two`` switches 0 -> 1
    once, and between the switch the backward's LDS grows with the graph."""
    two, n, switched = 0, 1, None
    last = None
    while True:
        p = _plan(F, H, L, C, n, 16, edges_per_node * n, 136)
        if p is None:
            break
        assert p["two"] >= two, (n, p)
        if p["two"] and not two:
            switched = n
        two = p["two"]
        if last is not None and last["two"] == p["two"]:
            assert p["bwd_lds"] >= last["bwd_lds"], (n, last, p)
        last = p
        n += 1
    assert n > 65, "the envelope reaches the 1024-thread class"
    if H == 64:      # the forward's 64 KB of weights end the envelope (n ~ 100) before three buffers stop fitting
        assert switched is None
    else:
        assert switched is not None and switched > 64, "the two-buffer backward is reached before the envelope ends"
    for m in range(n, n + 50):
        assert _plan(F, H, L, C, m, 16, edges_per_node * m, 136) is None, "the envelope does not reopen"


def test_double_buffered_weights_never_at_h64():
    saw_db = False
    for F, H, L, C in WIDTHS:
        for n, v, ell, evv in _shapes():
            for want in (False, True):
                p = _plan(F, H, L, C, n, v, ell, evv, want)
                if p is None:
                    continue
                if H == 64:
                    assert p["db"] == 0, (n, v, ell, evv)
                saw_db = saw_db or p["db"] == 1
    assert saw_db, "H <= 32 takes the double buffer where it fits"


def test_dropping_the_export_frees_forward_lds():
    """A shape whose forward cannot hold the export (csr_launch = 1) holds it once nothing asks for it, in no more LDS."""
    hit = 0
    for F, H, L, C in WIDTHS:
        for n, v, ell, evv in _shapes():
            a, b = _plan(F, H, L, C, n, v, ell, evv, True), _plan(F, H, L, C, n, v, ell, evv, False)
            if a is None:
                continue
            assert b["exp"] == 0 and b["csr_launch"] == 0 and b["two"] == a["two"] and b["bwd_lds"] == a["bwd_lds"]
            if a["exp"] and a["db"] == b["db"]:
                assert b["fwd_lds"] <= a["fwd_lds"], (n, v, ell, evv)
            hit += a["csr_launch"]
    assert hit, "some shape takes the separate CSR launch"


# --------------------------------------------------------------------------- #
# hscn_resident_launch_plan_ex: the same query over every stage-C launch shape
# --------------------------------------------------------------------------- #
def _recorder():
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import record_resident_plans
    return record_resident_plans


def _recorded():
    import os

    import numpy as np
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resident_launch_plans.npz")) as f:
        return f["rows"], [str(c) for c in f["columns"]]


def test_query_reproduces_the_recorded_launches():
    """tests/golden/resident_launch_plans.npz: what the launch functions of the commit before the planners did (template
    arguments, threads, LDS, the argument blocks' choice fields, read off their launch sites) -- row for row."""
    from graph_hscn import _hip
    R = _recorder()
    want, columns = _recorded()
    assert columns == list(R.columns())
    got = R.rows(_hip.resident_launch_plan_ex)
    assert got.shape == want.shape and got.dtype == want.dtype
    differ = (got != want).any(axis=1).nonzero()[0]
    assert differ.size == 0, [(want[i].tolist(), got[i].tolist()) for i in differ[:5]]


def test_selector_pair_rows_are_the_launch_plan():
    from graph_hscn import _hip
    lib = _hip.lib()
    buf = (ctypes.c_int32 * len(_hip.PLAN_FIELDS))()
    seen = set()
    for F, H, L, C in WIDTHS:
        for n, v, ell, evv in _shapes():
            for want in (0, 1):
                for i in range(len(buf)):
                    buf[i] = -7
                rc = lib.hscn_resident_launch_plan(F, H, L, C, n, v, ell, evv, want, buf)
                rc_ex, ex = _hip.resident_launch_plan_ex(_hip.LAUNCHES.index("pair"), F, H, L, C, n, v, ell, evv, want)
                assert rc == rc_ex and rc in (0, -3), (F, H, L, C, n, v, ell, evv, want)
                seen.add(rc)
                # the projection: the first seven fields; a refusal leaves the caller's buffer alone
                assert list(buf) == (ex[:len(buf)] if rc == 0 else [-7] * len(buf)), (F, H, L, C, n, v, ell, evv, want)
    assert seen == {0, -3}
    assert _hip.resident_launch_plan_ex(4, 9, 16, 3, 10, 100, 8, 200, 36)[0] == -1          # unknown launch
    assert _hip.resident_launch_plan_ex(-1, 9, 16, 3, 10, 100, 8, 200, 36)[0] == -1
    assert lib.hscn_resident_launch_plan_ex(0, 9, 16, 3, 10, 100, 8, 200, 36, 1, None) == -1


def test_launch_lds_covers_both_programs_and_fits_a_cu():
    """Every supported row: a launch's LDS is at least what each of its workgroup programs lays out for the argument
    block it is handed (the *_need fields: the kernels' own layout functions on the planned blocks), and at most a
    CU's 160 KB.  The needs themselves are tied to the plain pair's LDS where the blocks coincide."""
    from graph_hscn import _hip
    rows, columns = _recorded()
    ci = {c: i for i, c in enumerate(columns)}
    n_ok = 0
    for row in rows:
        r = {c: int(row[ci[c]]) for c in columns}
        if r["rc"] != 0:
            assert r["rc"] == -3 and not any(row[ci["rc"] + 1:]), r
            continue
        n_ok += 1
        assert 0 < r["fwd_local_need"] <= r["fwd_lds"] <= 160 * 1024, r
        assert 0 <= r["fwd_virtual_need"] <= r["fwd_lds"], r
        assert 0 <= r["bwd_local_need"] <= r["bwd_lds"] <= 160 * 1024 and 0 <= r["bwd_virtual_need"] <= r["bwd_lds"], r
        assert 0 <= r["csr_lds"] <= 160 * 1024 and (r["csr_lds"] > 0) == (r["csr_launch"] == 1), r
        launch = _hip.LAUNCHES[r["launch"]]
        virtual = launch in ("pair_virtual", "step_virtual")
        assert (r["fwd_virtual_need"] > 0) == virtual and (r["bwd_virtual_need"] > 0) == (launch == "pair_virtual"), r
        assert (r["bwd_lds"] > 0) == (r["bwd_local_need"] > 0) == launch.startswith("pair"), r
        if launch == "pair":
            assert r["fwd_local_need"] == r["fwd_lds"] and r["bwd_local_need"] == r["bwd_lds"], r
        if launch == "pair_virtual":
            # the export happens in exactly one place when it is wanted, nowhere when it is not
            assert r["exp"] + r["v_exp"] + r["csr_launch"] == r["want_export"], r
            # the local block is the plain forward's at the same export choice; the backward is the plain backward
            shape = (r["F"], r["H"], r["L"], r["C"], r["max_n"], r["max_v"], r["max_ell"], r["max_evv"])
            p = _hip.resident_launch_plan(*shape, bool(r["exp"]))
            assert (p["db"], p["exp"], p["fwd_lds"]) == (r["db"], r["exp"], r["fwd_local_need"]), (r, p)
            assert (p["two"], p["bwd_lds"]) == (r["two"], r["bwd_local_need"]), (r, p)
        if launch.startswith("step"):
            assert r["local_fixed"] <= (r["virtual_fixed"] if virtual else 1), r
            assert r["threads"] == 1024 or not (r["local_fixed"] or r["virtual_fixed"]), r
            assert r["v_acq"] == (1 if virtual and r["threads"] == 256 else 0), r
    assert n_ok > 1000
