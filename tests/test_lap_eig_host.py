"""The Laplacian-statistics launch (include/hscn.h: hscn_lap_eig_stats, csrc/lap_eig.hip) as far as it goes without a
device: the exports, the envelope, the argument checks that come before any launch, and the Python entry points'
refusals."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("hscn_lap_eig_supported", "hscn_lap_eig_lds_max_n", "hscn_lap_eig_workspace_bytes", "hscn_lap_eig_stats")

_BUF = ctypes.create_string_buffer(4096)
_HERE = ctypes.addressof(_BUF)


def test_exports_are_in_header_library_and_binding():
    from graph_hscn import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hscn.h")).read(), flags=re.S)
    lib = _hip.lib()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _hip._SIGNATURES, name
    assert lib.hscn_abi_version() == 24
    # the launch takes no `flags` word (tests/test_abi.py lists the entry points that do)
    assert not re.search(r"hscn_lap_eig_stats\s*\([^;{}]*\bint flags\s*,\s*void\* stream\)", src)


def test_envelope_and_workspace():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert lib.hscn_lap_eig_supported(512, 10) == 1
    assert lib.hscn_lap_eig_supported(513, 10) == 0
    assert lib.hscn_lap_eig_supported(30, 64) == 1
    assert lib.hscn_lap_eig_supported(30, 65) == 0
    assert lib.hscn_lap_eig_supported(0, 10) == 0 and lib.hscn_lap_eig_supported(30, 0) == 0
    m = lib.hscn_lap_eig_lds_max_n()
    assert 0 < m < 512
    assert lib.hscn_lap_eig_workspace_bytes(128, m) == 0
    assert lib.hscn_lap_eig_workspace_bytes(128, 1) == 0
    one, two = lib.hscn_lap_eig_workspace_bytes(1, m + 1), lib.hscn_lap_eig_workspace_bytes(2, m + 1)
    assert one > 0 and two == 2 * one
    # A and V^T of one 512-node graph: two matrices of 512 rows, rows padded to an odd length
    assert lib.hscn_lap_eig_workspace_bytes(1, 512) == 2 * 512 * 513 * 4
    assert lib.hscn_lap_eig_workspace_bytes(3, 512) > lib.hscn_lap_eig_workspace_bytes(3, 444) > 0


def _call(lib, **over):
    """A call whose arguments are all acceptable (host memory stands in for the pointers: the checks only compare them
    with NULL, and every variant below is refused before a launch) with ``over`` replacing some of them."""
    a = dict(edge_index=_HERE, E=4, nptr=_HERE, eptr=_HERE, N=6, B=2, max_n=3, lap_norm=1, is_undirected=1, max_freqs=4,
             eigvec_norm=1, eigvals=_HERE, eigvecs=_HERE, flag=_HERE, workspace=None, workspace_bytes=0, stream=None)
    a.update(over)
    return lib.hscn_lap_eig_stats(*a.values())


def test_argument_checks_come_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    for bad in (dict(E=-1), dict(N=-1), dict(B=-1), dict(max_n=-1), dict(max_freqs=0), dict(max_freqs=-3),
                dict(eigvals=None), dict(eigvecs=None), dict(flag=None), dict(nptr=None), dict(eptr=None),
                dict(edge_index=None), dict(lap_norm=3), dict(lap_norm=-1), dict(eigvec_norm=3), dict(eigvec_norm=-1)):
        assert _call(lib, **bad) == -1, bad
    m = lib.hscn_lap_eig_lds_max_n()
    need = lib.hscn_lap_eig_workspace_bytes(2, m + 1)
    assert _call(lib, max_n=m + 1, workspace=_HERE, workspace_bytes=need - 1) == -1
    assert _call(lib, max_n=m + 1, workspace=None, workspace_bytes=need) == -1
    # outside the envelope: HSCN_E_UNSUPPORTED, also before any launch
    assert _call(lib, max_n=513, workspace=_HERE, workspace_bytes=1 << 40) == -3
    assert _call(lib, max_freqs=65) == -3
    # nothing to do
    assert _call(lib, B=0) == 0 and _call(lib, N=0) == 0


def test_device_statistics_refuse_cpu_tensors():
    from graph_hscn.config.config import PEConfig
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.transform import compute_posenc_stats_device
    cfg = PEConfig(9, 16, 8, eigen_max_freqs=4)
    graphs = make_dataset("pcqm_contact", 2, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_posenc_stats_device(Batch.from_data_list(graphs), True, cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_posenc_stats_device(graphs, True, cfg, device="cpu")
    assert not hasattr(graphs[0], "eigvecs_sn")


def test_compute_posenc_refuses_an_unknown_stats_back_end():
    from graph_hscn.config.config import PEConfig
    from graph_hscn.train.train import compute_posenc

    class _NoLoader:
        def __iter__(self):
            raise AssertionError("the loaders were touched")

    cfg = PEConfig(9, 16, 8, eigen_max_freqs=4)
    with pytest.raises(ValueError, match="stats"):
        compute_posenc([_NoLoader()], None, 9, cfg, device="cuda", stats="bogus")
