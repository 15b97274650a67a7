"""The C-ABI library loads and exports every symbol include/hscn.h declares
(no compute calls: runs without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "hscn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hscn_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_surface():
    names = _declared()
    for must in ("hscn_csr_build", "hscn_spmm_csr_gcn", "hscn_spmm_csr_weighted", "hscn_gat_segment_fwd",
                 "hscn_gat_segment_bwd_dst", "hscn_gat_segment_bwd_src", "hscn_segment_mean_fwd",
                 "hscn_mincut_sparse_fwd", "hscn_mincut_sparse_bwd", "hscn_assign_argmax", "hscn_linear_fwd",
                 "hscn_resident_fwd", "hscn_resident_bwd"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from graph_hscn import _hip
    lib = _hip.lib()                       # raises if the .so is missing: there is no fallback
    for name in _declared():
        assert hasattr(lib, name), f"libhscn.so lacks {name}"
    assert lib.hscn_abi_version() == _hip.ABI_VERSION


def test_python_binding_covers_the_header():
    from graph_hscn import _hip
    assert sorted(_hip.exported_symbols()) == _declared()


def test_error_strings_and_argument_checks_without_a_gpu():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert lib.hscn_strerror(0) == b"ok"
    assert b"bad argument" in lib.hscn_strerror(-1)
    # argument validation happens before any launch
    assert lib.hscn_csr_build(None, None, -1, 4, 4, None, None, None, None, None, 0, None) == -1
    assert lib.hscn_resident_supported(9, 16, 3, 10, 444, 16, 1000, 136) == 1
    assert lib.hscn_resident_supported(9, 24, 3, 10, 444, 16, 1000, 136) == 0     # H must be 16/32/64
    assert lib.hscn_resident_supported(9, 16, 3, 10, 5000, 16, 10000, 136) == 0   # does not fit LDS
    assert lib.hscn_resident_param_count(9, 16, 3, 10) == 9 * 16 + 16 + 2 * (256 + 16) + 256 + 16 + 160 + 10


# The ten entry points that take `flags` (include/hscn.h, ABI 23): the bits each has a variant for, and a call that
# launches nothing yet gets past the flag check -- {argument position: value} over NULL pointers and zero sizes
# (_BUF: a host buffer standing in for a pointer the checks only compare with NULL) and what that call answers.
_STORE_F16, _GRAD_ACCUMULATE = 1, 2
_BUF = ctypes.create_string_buffer(512)
_HERE = ctypes.addressof(_BUF)
_FLAGGED = {
    # B = 0 (nothing to do: 0) at H = 16
    "hscn_resident_fwd": (_STORE_F16, {17: 16}, 0),
    "hscn_resident_fwd_with_virtual": (_STORE_F16, {8: 16, -3: _HERE}, 0),                       # -3: job
    "hscn_resident_bwd": (_STORE_F16 | _GRAD_ACCUMULATE, {8: 16}, 0),
    "hscn_resident_bwd_with_virtual": (_STORE_F16 | _GRAD_ACCUMULATE, {8: 16, -3: _HERE}, 0),
    "hscn_resident_train_step": (_STORE_F16 | _GRAD_ACCUMULATE, {}, 0),
    # one graph of widths F = H = K = 0: HSCN_E_UNSUPPORTED
    "hscn_scn_resident_fwd": (_STORE_F16, {6: 1}, -3),
    "hscn_scn_resident_bwd": (_STORE_F16, {6: 1}, -3),
    "hscn_scn_resident_train_step": (_STORE_F16, {6: 1}, -3),
    "hscn_scn_resident_train_epoch": (_STORE_F16, {4: 1}, -3),
    # B = 0 with the target, partials and grads it asks for first
    "hscn_mpnn_train_step": (_GRAD_ACCUMULATE, {15: _HERE, 20: _HERE, 21: _HERE}, 0),
}


def _blank_call(lib, name, flags, at):
    from graph_hscn import _hip
    types = _hip._SIGNATURES[name][1]
    assert types[-2] is ctypes.c_int and types[-1] is ctypes.c_void_p      # ..., int flags, void* stream
    args = [None if t is ctypes.c_void_p else 0 for t in types]
    for pos, v in at.items():
        args[pos] = v
    args[-2] = flags
    return getattr(lib, name)(*args)


def test_header_defines_the_flag_bits_the_binding_uses():
    from graph_hscn import _hip
    src = open(os.path.join(ROOT, "include", "hscn.h")).read()
    assert int(re.search(r"#define HSCN_STORE_F16 (\d+)", src).group(1)) == _hip.STORE_F16 == _STORE_F16
    assert int(re.search(r"#define HSCN_GRAD_ACCUMULATE (\d+)", src).group(1)) == _hip.GRAD_ACCUMULATE == _GRAD_ACCUMULATE
    assert int(re.search(r"#define HSCN_ABI_VERSION (\d+)", src).group(1)) == _hip.ABI_VERSION == 24
    # every entry point whose prototype has `int flags` is in the table above, and no other
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flagged = re.findall(r"\b(hscn_[a-z0-9_]+)\s*\([^;{}]*\bint flags\s*,\s*void\* stream\)", body)
    assert sorted(flagged) == sorted(_FLAGGED)


def test_flags_without_a_variant_are_refused_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    for name, (valid, at, rc) in _FLAGGED.items():
        assert rc != -1
        for ok in (0, _STORE_F16, _GRAD_ACCUMULATE, _STORE_F16 | _GRAD_ACCUMULATE):
            if ok & ~valid == 0:
                assert _blank_call(lib, name, ok, at) == rc, (name, ok)
        # an undefined bit, alone or beside a valid one, and a defined bit this entry point has no variant for
        for bad in (4, 1 << 30, -1, valid | 4) + tuple(b for b in (_STORE_F16, _GRAD_ACCUMULATE) if not valid & b):
            assert _blank_call(lib, name, bad, at) == -1, (name, bad)                  # HSCN_E_BADARG


def test_half_storage_is_unsupported_at_h64():
    from graph_hscn import _hip
    lib = _hip.lib()
    # float storage takes H = 64 (B = 0: nothing to do), half storage does not (H in {16, 32})
    for name, h_at in (("hscn_resident_fwd", 17), ("hscn_resident_bwd", 8), ("hscn_resident_fwd_with_virtual", 8),
                       ("hscn_resident_bwd_with_virtual", 8)):
        at = dict(_FLAGGED[name][1])
        for H, rc16 in ((16, 0), (32, 0), (64, -3)):                                   # HSCN_E_UNSUPPORTED
            at[h_at] = H
            assert _blank_call(lib, name, 0, at) == 0, (name, H)
            assert _blank_call(lib, name, _STORE_F16, at) == rc16, (name, H)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from graph_hscn import _hip
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "_LIB_PATH", str(tmp_path / "nope.so"))
    import pytest
    with pytest.raises(_hip.HipExtensionMissing):
        _hip.lib()


# What the five graph-resident entry points answer to calls that can never launch: every row keeps x_local NULL, so
# whatever the order of checks, a call that got past all the others is refused for it.  Argument positions by name
# (include/hscn.h); `job` / `structure`: a zeroed hscn_virtual_job / hscn_structure (_BUF) or NULL.
_RESIDENT_POS = {
    "hscn_resident_fwd": dict(B=15, F=16, H=17, L=18, C=19, max_n=27, max_ell=29),
    "hscn_resident_fwd_with_virtual": dict(B=6, F=7, H=8, L=9, C=10, max_n=17, max_ell=18, job=28),
    "hscn_resident_bwd": dict(B=6, F=7, H=8, L=9, C=10, max_n=23, max_ell=24),
    "hscn_resident_bwd_with_virtual": dict(B=6, F=7, H=8, L=9, C=10, max_n=23, max_ell=24, job=29),
    "hscn_resident_train_step": dict(B=6, F=7, H=8, L=9, C=10, max_n=17, max_ell=18, job=28, structure=29),
}
_FITS = dict(F=9, H=16, L=3, C=10, max_n=100, max_ell=200)          # inside every envelope


def _job_with_state():
    """A hscn_virtual_job whose six st_* members point somewhere (the forward with virtual workgroups asks for them)."""
    from graph_hscn.engine import _VirtualJob
    job = _VirtualJob()
    for n in ("st_rowptr_lv", "st_col_lv", "st_rowptr_vv", "st_col_vv", "st_dinv_v", "st_xv"):
        setattr(job, n, _HERE)
    return job


_JOB = _job_with_state()
_STATE = ctypes.addressof(_JOB)
# (row, arguments, flags, the codes of fwd / fwd_with_virtual / bwd / bwd_with_virtual / train_step): recorded from
# the commit before the launch planners, 0 = nothing to do, -1 = HSCN_E_BADARG, -3 = HSCN_E_UNSUPPORTED
_REFUSALS = [
    ("B < 0", dict(_FITS, B=-1, job=_HERE), 0, (-1, -1, -1, -1, -1)),
    ("B = 0", dict(_FITS, B=0, job=_HERE), 0, (0, 0, 0, 0, 0)),
    ("B = 0, all widths zero", dict(B=0, job=_HERE), 0, (0, 0, 0, 0, 0)),
    ("unsupported widths, B > 0", dict(_FITS, H=24, B=2, job=_HERE), 0, (-3, -1, -3, -3, -3)),
    ("unsupported widths, B > 0, job with state", dict(_FITS, H=24, B=2, job=_STATE), 0, (-3, -3, -3, -3, -3)),
    ("a graph beyond LDS, B > 0", dict(_FITS, max_n=5000, max_ell=10000, B=2, job=_STATE), 0, (-3, -3, -3, -3, -1)),
    ("supported widths, B > 0", dict(_FITS, B=2, job=_HERE), 0, (-1, -1, -1, -1, -1)),
    ("supported widths, B > 0, job with state", dict(_FITS, B=2, job=_STATE), 0, (-1, -1, -1, -1, -1)),
    ("missing job, B > 0", dict(_FITS, B=2), 0, (-1, -1, -1, -1, -1)),
    ("missing job, unsupported widths, B > 0", dict(_FITS, H=24, B=2), 0, (-3, -1, -3, -1, -3)),
    ("missing job, B = 0", dict(_FITS, B=0), 0, (0, -1, 0, -1, 0)),
    ("L < 2 with a job", dict(_FITS, L=1, B=2, job=_HERE), 0, (-1, -1, -1, -1, -1)),
    ("L < 2 with a job with state, unsupported widths", dict(_FITS, H=24, L=1, B=2, job=_STATE), 0, (-3, -1, -3, -3, -3)),
    ("structure with a missing member, B = 0", dict(_FITS, B=0, job=_HERE, structure=_HERE), 0, (0, 0, 0, 0, -1)),
    ("structure with a missing member, no job, B = 0", dict(_FITS, B=0, structure=_HERE), 0, (0, -1, 0, -1, -1)),
    ("half storage at H = 64, B > 0", dict(_FITS, H=64, B=2, job=_STATE), _STORE_F16, (-3, -3, -3, -3, -3)),
    ("half storage at H = 64, B = 0", dict(_FITS, H=64, B=0, job=_STATE), _STORE_F16, (-3, -3, -3, -3, 0)),
    ("float storage at H = 64, B > 0", dict(_FITS, H=64, B=2, job=_STATE), 0, (-1, -1, -1, -1, -3)),
]


def _refusal_codes(lib, args, flags):
    out = []
    for name, pos in _RESIDENT_POS.items():
        at = {pos[k]: v for k, v in args.items() if k in pos}
        assert 0 not in at                                                         # x_local stays NULL
        out.append(_blank_call(lib, name, flags, at))
    return tuple(out)


def test_resident_entry_points_refuse_as_recorded():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert list(_RESIDENT_POS) == [n for n in _FLAGGED if n.startswith("hscn_resident_")]
    for row, args, flags, codes in _REFUSALS:
        assert _refusal_codes(lib, args, flags) == codes, row


# What every entry point whose launch asks for dynamic LDS answers to calls that can never launch: recorded from the
# commit before they shared one launch helper.  Arguments by name (include/hscn.h) over NULL pointers and zero sizes;
# _HERE stands in for a pointer the checks only compare with NULL (as a params_host / layer_params_host it is a table
# of NULL entries).  Every row leaves a required pointer or member NULL, asks for nothing (B = 0, visits = 0) or asks
# for more LDS than a CU has, so whatever the order of checks no row reaches a launch.
def _positions(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hscn.h")).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^;{}]*)\)\s*;" % name, src).group(1).split(",")
    return {p.split()[-1].lstrip("*"): i for i, p in enumerate(params)}


def _named_call(lib, name, kw):
    from graph_hscn import _hip
    pos = _positions(name)
    args = [None if t is ctypes.c_void_p else 0 for t in _hip._SIGNATURES[name][1]]
    for k, v in kw.items():
        args[pos[k]] = v
    return getattr(lib, name)(*args)


def _adam(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, **missing):
    """A hscn_adam whose five pointers point somewhere, except the ones named in `missing`."""
    from graph_hscn.optim import _AdamC
    o = _AdamC(beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay)
    for n in ("exp_avg", "exp_avg_sq", "step", "beta_pows", "lr"):
        setattr(o, n, None if n in missing else _HERE)
    _KEEP.append(o)
    return ctypes.addressof(o)


def _scn_structure(ready=1, **missing):
    """A hscn_scn_structure with every array but xpad (optional), except the ones named in `missing`."""
    from graph_hscn.step import _ScnStructC
    c = _ScnStructC(ready=ready)
    for n in ("rowptr_d", "col_d", "rowptr_s", "col_s", "agg", "dout"):
        setattr(c, n, None if n in missing else _HERE)
    _KEEP.append(c)
    return ctypes.addressof(c)


_KEEP = []
_NAN = float("nan")
_SCN = dict(N=10, B=1, F=9, H=16, K=8, max_n=100, max_e=200)                                  # inside the envelope
_SCN_W = dict(W_rel=_HERE, b_rel=_HERE, W_root=_HERE, W_mlp=_HERE, b_mlp=_HERE, nptr=_HERE, eptr=_HERE)
_SCN_FWD_ALL = dict(_SCN, **_SCN_W, x=_HERE, S=_HERE, y=_HERE, stats=_HERE, ss=_HERE, losses=_HERE)
_SCN_EPOCH = dict(N=10, G=2, visits=0, F=9, H=16, K=8, max_n=100, max_e=200)
_SCN_EPOCH_ALL = dict(_SCN_EPOCH, **_SCN_W, x=_HERE, grads=_HERE, stats=_HERE, losses=_HERE, ticket=_HERE)
_MPNN = dict(B=2, F=9, H=16, L=3, C=10, max_n=100, max_ell=200)
_MPNN_P = dict(ptr32=_HERE, eptr32=_HERE, params_host=_HERE, pred=_HERE)
_MPNN_T = dict(target=_HERE, partials=_HERE, grads=_HERE)
_VL = dict(B=2, F=9, H=16, L=2, C=10, max_n=100, max_v=8, max_ell=200, max_evv=36)
_VL_P = dict(lptr=_HERE, vptr=_HERE, eptr_ll=_HERE, eptr_vv=_HERE, eptr_lv=_HERE, layer_params_host=_HERE, W1=_HERE,
             b1=_HERE, W2=_HERE, b2=_HERE, pred=_HERE)
_SN = dict(B=2, F=9, K=8, hidden=16, phi_out=8, layers=2, post_layers=2, dim_pe=8, dim_x=9, max_n=100, max_e=200)
_SN_P = dict(ptr32=_HERE, eptr32=_HERE, params_host=_HERE)
_LE = dict(B=1, N=1, max_n=100, max_freqs=8)
_LE_P = dict(nptr=_HERE, eptr=_HERE, eigvals=_HERE, eigvecs=_HERE, flag=_HERE)
_MC_F = dict(logits=_HERE, rowptr=_HERE, col=_HERE, node_ptr=_HERE, S=_HERE, stats=_HERE, ss=_HERE, losses=_HERE)
_MC_B = dict(S=_HERE, stats=_HERE, ss=_HERE, rowptr=_HERE, col=_HERE, rowptr_t=_HERE, col_t=_HERE, node_ptr=_HERE,
             g_losses=_HERE, g_logits=_HERE)
_NH = dict(N=100, H=32, C=10)
_NH_P = dict(x=_HERE, W1=_HERE, b1=_HERE, W2=_HERE, b2=_HERE, g_pred=_HERE, gW1=_HERE, gb1=_HERE, gW2=_HERE, gb2=_HERE,
             workspace=_HERE)
_AP_P = dict(y_true=_HERE, y_score=_HERE, ap=_HERE, valid=_HERE, result=_HERE, flags=_HERE, workspace=_HERE)
_LIN = dict(x=_HERE, W=_HERE, y=_HERE, rows=1)
_LDS_REFUSALS = [
    # stage A: forward
    ("hscn_scn_resident_fwd", "B < 1", dict(_SCN, B=0), -1),
    ("hscn_scn_resident_fwd", "B < 1 and unsupported widths", dict(_SCN, B=0, H=24), -1),
    ("hscn_scn_resident_fwd", "unsupported widths and NULL pointers", dict(_SCN, H=24), -3),
    ("hscn_scn_resident_fwd", "H = 64", dict(_SCN, H=64), -3),
    ("hscn_scn_resident_fwd", "F beyond 16", dict(_SCN, F=17), -3),
    ("hscn_scn_resident_fwd", "a graph beyond LDS", dict(_SCN, max_n=5000, max_e=20000), -3),
    ("hscn_scn_resident_fwd", "NULL pointers", dict(_SCN), -1),
    ("hscn_scn_resident_fwd", "edges without edge_index", dict(_SCN_FWD_ALL, E=5), -1),
    ("hscn_scn_resident_fwd", "one export array of six", dict(_SCN_FWD_ALL, ex_rowptr_d=_HERE), -1),
    ("hscn_scn_resident_fwd", "five export arrays of six",
     dict(_SCN_FWD_ALL, ex_rowptr_d=_HERE, ex_col_d=_HERE, ex_rowptr_s=_HERE, ex_col_s=_HERE, ex_agg=_HERE), -1),
    ("hscn_scn_resident_fwd", "export arrays in part, unsupported widths", dict(_SCN_FWD_ALL, H=24, ex_agg=_HERE), -3),
    # stage A: backward
    ("hscn_scn_resident_bwd", "B < 1", dict(_SCN, B=0), -1),
    ("hscn_scn_resident_bwd", "unsupported widths and NULL pointers", dict(_SCN, H=24), -3),
    ("hscn_scn_resident_bwd", "a graph beyond LDS", dict(_SCN, max_n=5000, max_e=20000), -3),
    ("hscn_scn_resident_bwd", "NULL pointers", dict(_SCN), -1),
    ("hscn_scn_resident_bwd", "negative E", dict(_SCN, E=-1, H=24), -1),
    # stage A: one-launch step (H = 24 behind a check that passes answers -3, so the row shows the check passed)
    ("hscn_scn_resident_train_step", "B < 1", dict(_SCN, B=0), -1),
    ("hscn_scn_resident_train_step", "unsupported widths and NULL pointers", dict(_SCN, H=24), -3),
    ("hscn_scn_resident_train_step", "K not a multiple of 4", dict(_SCN, K=6), -3),
    ("hscn_scn_resident_train_step", "max_n beyond 512", dict(_SCN, max_n=513, max_e=100), -3),
    ("hscn_scn_resident_train_step", "a graph beyond LDS", dict(_SCN, max_n=500, max_e=20000), -3),
    ("hscn_scn_resident_train_step", "NULL pointers", dict(_SCN), -1),
    ("hscn_scn_resident_train_step", "structure without members, unsupported widths", dict(_SCN, H=24, cache=_HERE), -1),
    ("hscn_scn_resident_train_step", "whole structure, unsupported widths", dict(_SCN, H=24, cache=_scn_structure()), -3),
    ("hscn_scn_resident_train_step", "structure without agg", dict(_SCN, H=24, cache=_scn_structure(agg=1)), -1),
    ("hscn_scn_resident_train_step", "structure without columns, E = 0",
     dict(_SCN, H=24, cache=_scn_structure(col_d=1, col_s=1)), -3),
    ("hscn_scn_resident_train_step", "structure without columns, E > 0",
     dict(_SCN, H=24, E=5, cache=_scn_structure(col_d=1, col_s=1)), -1),
    ("hscn_scn_resident_train_step", "structure without col_s, E > 0", dict(_SCN, H=24, E=5, cache=_scn_structure(col_s=1)), -1),
    ("hscn_scn_resident_train_step", "structure not ready, unsupported widths",
     dict(_SCN, H=24, cache=_scn_structure(ready=0)), -3),
    ("hscn_scn_resident_train_step", "optimizer, B = 1, unsupported widths", dict(_SCN, H=24, opt=_adam()), -3),
    ("hscn_scn_resident_train_step", "optimizer, B = 2", dict(_SCN, H=24, B=2, opt=_adam()), -1),
    ("hscn_scn_resident_train_step", "optimizer without members", dict(_SCN, H=24, opt=_HERE), -1),
    ("hscn_scn_resident_train_step", "optimizer without lr", dict(_SCN, H=24, opt=_adam(lr=1)), -1),
    ("hscn_scn_resident_train_step", "optimizer without step", dict(_SCN, H=24, opt=_adam(step=1)), -1),
    ("hscn_scn_resident_train_step", "beta1 = 1", dict(_SCN, H=24, opt=_adam(beta1=1.0)), -1),
    ("hscn_scn_resident_train_step", "beta1 = 0", dict(_SCN, H=24, opt=_adam(beta1=0.0)), -3),
    ("hscn_scn_resident_train_step", "beta2 < 0", dict(_SCN, H=24, opt=_adam(beta2=-0.5)), -1),
    ("hscn_scn_resident_train_step", "beta2 NaN", dict(_SCN, H=24, opt=_adam(beta2=_NAN)), -1),
    ("hscn_scn_resident_train_step", "eps < 0", dict(_SCN, H=24, opt=_adam(eps=-1e-8)), -1),
    ("hscn_scn_resident_train_step", "eps = 0", dict(_SCN, H=24, opt=_adam(eps=0.0)), -3),
    ("hscn_scn_resident_train_step", "weight_decay < 0", dict(_SCN, H=24, opt=_adam(weight_decay=-0.1)), -1),
    ("hscn_scn_resident_train_step", "weight_decay NaN", dict(_SCN, H=24, opt=_adam(weight_decay=_NAN)), -1),
    ("hscn_scn_resident_train_step", "optimizer and structure, NULL pointers",
     dict(_SCN, opt=_adam(), cache=_scn_structure()), -1),
    # stage A: the epoch (visits = 0 where every check passes: nothing to launch)
    ("hscn_scn_resident_train_epoch", "G < 1", dict(_SCN_EPOCH, G=0), -1),
    ("hscn_scn_resident_train_epoch", "visits < 0", dict(_SCN_EPOCH, visits=-1), -1),
    ("hscn_scn_resident_train_epoch", "unsupported widths and NULL pointers", dict(_SCN_EPOCH, H=24), -3),
    ("hscn_scn_resident_train_epoch", "a graph beyond LDS", dict(_SCN_EPOCH, max_n=500, max_e=20000), -3),
    ("hscn_scn_resident_train_epoch", "NULL pointers", dict(_SCN_EPOCH), -1),
    ("hscn_scn_resident_train_epoch", "no structure", dict(_SCN_EPOCH_ALL, opt=_adam()), -1),
    ("hscn_scn_resident_train_epoch", "no optimizer", dict(_SCN_EPOCH_ALL, cache=_scn_structure()), -1),
    ("hscn_scn_resident_train_epoch", "structure not ready", dict(_SCN_EPOCH_ALL, opt=_adam(), cache=_scn_structure(ready=0)), -1),
    ("hscn_scn_resident_train_epoch", "structure without columns",
     dict(_SCN_EPOCH_ALL, opt=_adam(), cache=_scn_structure(col_d=1, col_s=1)), -1),
    ("hscn_scn_resident_train_epoch", "structure without col_d", dict(_SCN_EPOCH_ALL, opt=_adam(), cache=_scn_structure(col_d=1)), -1),
    ("hscn_scn_resident_train_epoch", "structure without dout", dict(_SCN_EPOCH_ALL, opt=_adam(), cache=_scn_structure(dout=1)), -1),
    ("hscn_scn_resident_train_epoch", "optimizer without beta_pows",
     dict(_SCN_EPOCH_ALL, opt=_adam(beta_pows=1), cache=_scn_structure()), -1),
    ("hscn_scn_resident_train_epoch", "beta1 = 1", dict(_SCN_EPOCH_ALL, opt=_adam(beta1=1.0), cache=_scn_structure()), -1),
    ("hscn_scn_resident_train_epoch", "eps NaN", dict(_SCN_EPOCH_ALL, opt=_adam(eps=_NAN), cache=_scn_structure()), -1),
    ("hscn_scn_resident_train_epoch", "weight_decay < 0",
     dict(_SCN_EPOCH_ALL, opt=_adam(weight_decay=-1.0), cache=_scn_structure()), -1),
    ("hscn_scn_resident_train_epoch", "everything given, no visits", dict(_SCN_EPOCH_ALL, opt=_adam(), cache=_scn_structure()), 0),
    ("hscn_scn_resident_train_epoch", "bad optimizer, unsupported widths",
     dict(_SCN_EPOCH_ALL, H=24, opt=_adam(beta1=1.0), cache=_scn_structure()), -3),
    # MPNN baseline
    ("hscn_mpnn_train_step", "B < 0", dict(_MPNN, **_MPNN_T, B=-1), -1),
    ("hscn_mpnn_train_step", "B = 0", dict(_MPNN, **_MPNN_T, B=0), 0),
    ("hscn_mpnn_train_step", "B = 0 without a target", dict(_MPNN, B=0), -1),
    ("hscn_mpnn_train_step", "p = 1", dict(_MPNN, **_MPNN_T, p=1.0), -1),
    ("hscn_mpnn_train_step", "unsupported widths and NULL pointers", dict(_MPNN, **_MPNN_T, H=24), -1),
    ("hscn_mpnn_train_step", "unsupported widths", dict(_MPNN, **_MPNN_T, **_MPNN_P, H=24), -3),
    ("hscn_mpnn_train_step", "H = 64", dict(_MPNN, **_MPNN_T, **_MPNN_P, H=64), -3),
    ("hscn_mpnn_train_step", "a graph beyond LDS", dict(_MPNN, **_MPNN_T, **_MPNN_P, max_n=5000, max_ell=10000), -3),
    ("hscn_mpnn_train_step", "unknown act", dict(_MPNN, **_MPNN_T, **_MPNN_P, H=24, act=7), -1),
    ("hscn_mpnn_train_step", "unknown loss", dict(_MPNN, **_MPNN_T, **_MPNN_P, H=24, loss_kind=2), -1),
    ("hscn_mpnn_train_step", "a table of NULL parameters", dict(_MPNN, **_MPNN_T, **_MPNN_P), -1),
    ("hscn_mpnn_forward", "B < 0", dict(_MPNN, B=-1), -1),
    ("hscn_mpnn_forward", "B = 0", dict(_MPNN, B=0), 0),
    ("hscn_mpnn_forward", "loss without loss_rows", dict(_MPNN, B=0, loss=_HERE, target=_HERE), -1),
    ("hscn_mpnn_forward", "unsupported widths and NULL pointers", dict(_MPNN, H=24), -1),
    ("hscn_mpnn_forward", "unsupported widths", dict(_MPNN, **_MPNN_P, H=24), -3),
    ("hscn_mpnn_forward", "a graph beyond LDS", dict(_MPNN, **_MPNN_P, max_n=5000, max_ell=10000), -3),
    ("hscn_mpnn_forward", "a table of NULL parameters", dict(_MPNN, **_MPNN_P), -1),
    # virtual -> local step
    ("hscn_vl_train_step", "B < 0", dict(_VL, **_MPNN_T, B=-1), -1),
    ("hscn_vl_train_step", "B = 0", dict(_VL, B=0), 0),
    ("hscn_vl_train_step", "no target", dict(_VL, **_VL_P), -1),
    ("hscn_vl_train_step", "unsupported widths and NULL pointers", dict(_VL, **_MPNN_T, H=24), -1),
    ("hscn_vl_train_step", "unsupported widths", dict(_VL, **_MPNN_T, **_VL_P, H=24), -3),
    ("hscn_vl_train_step", "a graph beyond LDS", dict(_VL, **_MPNN_T, **_VL_P, max_n=5000, max_ell=10000), -3),
    ("hscn_vl_train_step", "virtual nodes beyond LDS", dict(_VL, **_MPNN_T, **_VL_P, max_v=2000, max_evv=4000), -3),
    ("hscn_vl_train_step", "a table of NULL parameters", dict(_VL, **_MPNN_T, **_VL_P), -1),
    ("hscn_vl_forward", "B < 0", dict(_VL, B=-1), -1),
    ("hscn_vl_forward", "B = 0", dict(_VL, B=0), 0),
    ("hscn_vl_forward", "loss without loss_rows", dict(_VL, B=0, loss=_HERE, target=_HERE), -1),
    ("hscn_vl_forward", "unsupported widths and NULL pointers", dict(_VL, H=24), -1),
    ("hscn_vl_forward", "unsupported widths", dict(_VL, **_VL_P, H=24), -3),
    ("hscn_vl_forward", "a graph beyond LDS", dict(_VL, **_VL_P, max_n=5000, max_ell=10000), -3),
    ("hscn_vl_forward", "a table of NULL parameters", dict(_VL, **_VL_P), -1),
    # SignNet encoder, Laplacian statistics
    ("hscn_signnet_encode", "B < 0", dict(_SN, **_SN_P, B=-1), -1),
    ("hscn_signnet_encode", "NULL pointers", dict(_SN), -1),
    ("hscn_signnet_encode", "F < 1", dict(_SN, **_SN_P, F=0), -1),
    ("hscn_signnet_encode", "dim_x != F without expand_x", dict(_SN, **_SN_P, dim_x=16), -1),
    ("hscn_signnet_encode", "hidden beyond 64", dict(_SN, **_SN_P, hidden=65), -3),
    ("hscn_signnet_encode", "hidden beyond 64 and NULL pointers", dict(_SN, hidden=65), -1),
    ("hscn_signnet_encode", "a graph beyond LDS", dict(_SN, **_SN_P, max_n=5000, max_e=20000), -3),
    ("hscn_signnet_encode", "a table of NULL parameters", dict(_SN, **_SN_P), -1),
    ("hscn_signnet_encode", "a table of NULL parameters, B = 0", dict(_SN, **_SN_P, B=0), -1),
    ("hscn_lap_eig_stats", "B < 0", dict(_LE, **_LE_P, B=-1), -1),
    ("hscn_lap_eig_stats", "max_freqs < 1", dict(_LE, **_LE_P, max_freqs=0), -1),
    ("hscn_lap_eig_stats", "NULL pointers", dict(_LE), -1),
    ("hscn_lap_eig_stats", "NULL pointers, B = 0", dict(_LE, B=0), -1),
    ("hscn_lap_eig_stats", "B = 0", dict(_LE, **_LE_P, B=0), 0),
    ("hscn_lap_eig_stats", "B = 0, unsupported sizes", dict(_LE, **_LE_P, B=0, max_n=513), 0),
    ("hscn_lap_eig_stats", "max_n beyond 512", dict(_LE, **_LE_P, max_n=513), -3),
    ("hscn_lap_eig_stats", "max_freqs beyond 64", dict(_LE, **_LE_P, max_freqs=65), -3),
    ("hscn_lap_eig_stats", "a graph beyond LDS without its workspace", dict(_LE, **_LE_P, max_n=512), -1),
    # MinCUT, node head, average precision, linear
    ("hscn_mincut_sparse_fwd", "no graphs", dict(_MC_F, K=8), -1),
    ("hscn_mincut_sparse_fwd", "K beyond 256", dict(_MC_F, num_graphs=1, K=257), -1),
    ("hscn_mincut_sparse_fwd", "NULL pointers", dict(num_graphs=1, K=8), -1),
    ("hscn_mincut_sparse_fwd", "NULL pointers, K beyond LDS", dict(num_graphs=1, K=256), -1),
    ("hscn_mincut_sparse_fwd", "K beyond LDS, no nodes", dict(_MC_F, num_graphs=1, K=256), -3),
    ("hscn_mincut_sparse_bwd", "no graphs", dict(_MC_B, K=8), -1),
    ("hscn_mincut_sparse_bwd", "K < 1", dict(_MC_B, num_graphs=1), -1),
    ("hscn_mincut_sparse_bwd", "NULL pointers", dict(num_graphs=1, K=8), -1),
    ("hscn_mincut_sparse_bwd", "NULL pointers, K beyond LDS", dict(num_graphs=1, K=256), -1),
    ("hscn_mincut_sparse_bwd", "K beyond LDS", dict(_MC_B, num_graphs=1, K=256), -3),
    ("hscn_node_head_bwd", "N < 1", dict(_NH, **_NH_P, N=0), -1),
    ("hscn_node_head_bwd", "NULL pointers", dict(_NH), -1),
    ("hscn_node_head_bwd", "unsupported widths and NULL pointers", dict(_NH, H=24), -1),
    ("hscn_node_head_bwd", "unsupported widths", dict(_NH, **_NH_P, H=24), -3),
    ("hscn_node_head_bwd", "C beyond 64", dict(_NH, **_NH_P, C=65), -3),
    ("hscn_node_head_bwd", "unknown act", dict(_NH, **_NH_P, H=24, act=4), -1),
    ("hscn_node_head_bwd", "no room in the workspace", dict(_NH, **_NH_P), -2),
    ("hscn_node_head_bwd", "no room in the workspace, H = C = 64", dict(_NH, **_NH_P, H=64, C=64), -2),
    ("hscn_average_precision", "G < 1", dict(_AP_P, C=10), -1),
    ("hscn_average_precision", "NULL pointers", dict(G=5000, C=10), -1),
    ("hscn_average_precision", "no room in the workspace", dict(_AP_P, G=5000, C=10), -2),
    ("hscn_average_precision", "no room in the workspace, keys beyond LDS", dict(_AP_P, G=20000, C=10), -2),
    ("hscn_linear_fwd", "rows < 0", dict(_LIN, rows=-1, in_f=16, out_f=16), -1),
    ("hscn_linear_fwd", "in_f < 1", dict(_LIN, out_f=16), -1),
    ("hscn_linear_fwd", "NULL W", dict(_LIN, W=None, in_f=16, out_f=16), -1),
    ("hscn_linear_fwd", "NULL x", dict(_LIN, x=None, in_f=16, out_f=16), -1),
    ("hscn_linear_fwd", "x2 without W2", dict(_LIN, x2=_HERE, in_f=16, out_f=16), -1),
    ("hscn_linear_fwd", "no rows", dict(W=_HERE, in_f=16, out_f=16), 0),
    ("hscn_linear_fwd", "no rows, weights beyond LDS", dict(W=_HERE, in_f=1024, out_f=64), 0),
    ("hscn_linear_fwd", "a row wider than a workgroup", dict(_LIN, in_f=4, out_f=8192), -3),
    ("hscn_linear_fwd", "weights beyond LDS", dict(_LIN, in_f=1024, out_f=64), -3),
    ("hscn_linear_fwd", "two weight matrices beyond LDS", dict(_LIN, x2=_HERE, W2=_HERE, in_f=512, out_f=64), -3),
    ("hscn_linear_fwd", "unfused attention with a bias", dict(_LIN, att=_HERE, a_out=_HERE, bias=_HERE, in_f=16, out_f=12), -3),
]


def test_lds_entry_points_refuse_as_recorded():
    from graph_hscn import _hip
    lib = _hip.lib()
    covered = {name for name, _, _, _ in _LDS_REFUSALS}
    assert covered == {"hscn_scn_resident_fwd", "hscn_scn_resident_bwd", "hscn_scn_resident_train_step",
                       "hscn_scn_resident_train_epoch", "hscn_mpnn_train_step", "hscn_mpnn_forward",
                       "hscn_vl_train_step", "hscn_vl_forward", "hscn_signnet_encode", "hscn_lap_eig_stats",
                       "hscn_mincut_sparse_fwd", "hscn_mincut_sparse_bwd", "hscn_node_head_bwd",
                       "hscn_average_precision", "hscn_linear_fwd"}
    for name, row, kw, code in _LDS_REFUSALS:
        assert _named_call(lib, name, kw) == code, (name, row)
