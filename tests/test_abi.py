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
