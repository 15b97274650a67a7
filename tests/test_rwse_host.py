"""The random-walk structural encoding (include/hscn.h: hscn_rwse_stats, csrc/rwse.hip, graph_hscn/transform/rwse.py,
graph_hscn/encoder/rwse.py) as far as it goes without a device: the exports, the envelope, the argument checks that
come before any launch, the host path against values worked by hand, the config and the encoder's construction."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("hscn_rwse_supported", "hscn_rwse_tile", "hscn_rwse_stats")

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


def test_envelope_and_tile():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert lib.hscn_rwse_supported(512, 64) == 1
    assert lib.hscn_rwse_supported(1, 1) == 1
    assert lib.hscn_rwse_supported(0, 20) == 0
    assert lib.hscn_rwse_supported(513, 20) == 0
    assert lib.hscn_rwse_supported(30, 65) == 0
    assert lib.hscn_rwse_supported(30, 0) == 0
    T = lib.hscn_rwse_tile()
    assert T >= 1 and 2 * 512 * T * 4 <= 160 * 1024            # the ping-pong pair of the largest graph fits a CU's LDS


def _call(lib, **over):
    """A call whose arguments are all acceptable (host memory stands in for the pointers: the checks only compare them
    with NULL, and every variant below is refused before a launch) with ``over`` replacing some of them."""
    a = dict(rowptr=_HERE, col=_HERE, nptr=_HERE, N=6, B=2, max_n=3, ksteps=4, rw=_HERE, flag=_HERE, stream=None)
    a.update(over)
    return lib.hscn_rwse_stats(*a.values())


def test_argument_checks_come_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    for bad in (dict(rowptr=None), dict(col=None), dict(nptr=None), dict(rw=None), dict(flag=None), dict(N=-1),
                dict(B=-1), dict(max_n=-1), dict(ksteps=0), dict(ksteps=-2)):
        assert _call(lib, **bad) == -1, bad                    # HSCN_E_BADARG
    for outside in (dict(max_n=513), dict(max_n=0), dict(ksteps=65)):
        assert _call(lib, **outside) == -3, outside            # HSCN_E_UNSUPPORTED
    assert _call(lib, B=0) == 0 and _call(lib, N=0) == 0       # nothing to do


def _rw(edges, n, K, is_undirected=True):
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.data import Data
    from graph_hscn.transform import compute_rwse_stats
    ei = torch.tensor(edges, dtype=torch.int64).reshape(-1, 2).t().contiguous()
    d = Data(x=torch.zeros(n, 1), edge_index=ei, num_nodes=n)
    out = compute_rwse_stats(d, is_undirected, RWSEConfig(1, 4, 2, ksteps=K))
    assert out is d and d.rwse.dtype == torch.float32 and tuple(d.rwse.shape) == (n, K)
    return d.rwse


def _eq(got, want):
    return torch.allclose(got, torch.tensor(want, dtype=torch.float32), rtol=0, atol=1e-6)


def test_host_path_against_values_worked_by_hand():
    # path 0 - 1 - 2: the ends return after 2 steps with 1/2 (0 -> 1 -> 0), the middle with 1; bipartite: odd steps 0
    assert _eq(_rw([(0, 1), (1, 0), (1, 2), (2, 1)], 3, 4), [[0, .5, 0, .5], [0, 1, 0, 1], [0, .5, 0, .5]])
    # triangle: P = (J - I) / 2; P^2 = (J + I) / 4, diagonal 1/2; P^3 = (3 J - I) / 8, diagonal 1/4
    tri = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]
    assert _eq(_rw(tri, 3, 3), [[0, .5, .25]] * 3)
    # node 0 with a self loop and the edge 0 <-> 1: P = [[1/2, 1/2], [1, 0]]; P^2 = [[3/4, 1/4], [1/2, 1/2]];
    # P^3 = [[5/8, 3/8], [3/4, 1/4]]
    assert _eq(_rw([(0, 0), (0, 1), (1, 0)], 2, 3), [[.5, .75, .625], [0, .5, .25]])
    # the edge 0 -> 1 listed twice beside 0 -> 2, all with their reverses once: A[0] = [0, 2, 1], deg 3;
    # (P^2)[0, 0] = 2/3 + 1/3 = 1, (P^2)[1, 1] = 2/3, (P^2)[2, 2] = 1/3
    dup = [(0, 1), (0, 1), (0, 2), (1, 0), (2, 0)]
    assert _eq(_rw(dup, 3, 2), [[0, 1], [0, 2 / 3], [0, 1 / 3]])
    # an isolated node beside an edge: zeros
    assert _eq(_rw([(0, 1), (1, 0)], 3, 2), [[0, 1], [0, 1], [0, 0]])
    # a single node: without edges zeros, with its loop ones
    assert _eq(_rw([], 1, 3), [[0, 0, 0]])
    assert _eq(_rw([(0, 0)], 1, 3), [[1, 1, 1]])
    # one-directional list 0 -> 1 -> 2: as given nothing returns; is_undirected=False makes it the path above
    assert _eq(_rw([(0, 1), (1, 2)], 3, 2), [[0, 0]] * 3)
    assert _eq(_rw([(0, 1), (1, 2)], 3, 4, is_undirected=False), [[0, .5, 0, .5], [0, 1, 0, 1], [0, .5, 0, .5]])
    # is_undirected=False merges duplicates: the doubled edge counts once
    assert _eq(_rw(dup, 3, 2, is_undirected=False), [[0, 1], [0, .5], [0, .5]])


def test_config_validation():
    from graph_hscn.config.config import RWSEConfig
    c = RWSEConfig(9, 16, 8)
    assert (c.ksteps, c.model, c.layers, c.raw_norm, c.pass_as_var) == (20, "linear", 1, "none", False)
    RWSEConfig(9, 16, 15, ksteps=1, model="mlp", layers=3, raw_norm="batchnorm", pass_as_var=True)
    for bad in (dict(ksteps=0), dict(model="MLP"), dict(model="deepset"), dict(layers=0), dict(raw_norm="layernorm"),
                dict(dim_pe=16), dict(dim_pe=17)):
        kw = dict(dim_in=9, dim_emb=16, dim_pe=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            RWSEConfig(**kw)


def _shapes(module):
    return {n: tuple(p.shape) for n, p in module.named_parameters()}


def test_encoder_parameter_names_and_shapes():
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.encoder import RWSENodeEncoder
    from graph_hscn.nn import BatchNorm1d, Linear
    x_part = {"linear_x.weight": (8, 9), "linear_x.bias": (8,)}
    enc = RWSENodeEncoder(RWSEConfig(9, 16, 8, ksteps=20), 9, 16)
    assert _shapes(enc) == {**x_part, "pe_encoder.0.weight": (8, 20), "pe_encoder.0.bias": (8,)}
    assert isinstance(enc.linear_x, Linear) and isinstance(enc.pe_encoder[0], Linear) and enc.raw_norm is None
    assert enc._act == "identity"
    enc = RWSENodeEncoder(RWSEConfig(9, 16, 8, ksteps=12, model="mlp", layers=1), 9, 16)
    assert _shapes(enc) == {**x_part, "pe_encoder.0.weight": (8, 12), "pe_encoder.0.bias": (8,)}
    assert enc._act == "relu"
    enc = RWSENodeEncoder(RWSEConfig(9, 16, 8, ksteps=12, model="mlp", layers=2), 9, 16)
    assert _shapes(enc) == {**x_part, "pe_encoder.0.weight": (16, 12), "pe_encoder.0.bias": (16,),
                            "pe_encoder.1.weight": (8, 16), "pe_encoder.1.bias": (8,)}
    enc = RWSENodeEncoder(RWSEConfig(9, 16, 8, ksteps=12, model="mlp", layers=3, raw_norm="batchnorm"), 9, 16,
                          expand_x=False)
    assert _shapes(enc) == {"raw_norm.weight": (12,), "raw_norm.bias": (12,),
                            "pe_encoder.0.weight": (16, 12), "pe_encoder.0.bias": (16,),
                            "pe_encoder.1.weight": (16, 16), "pe_encoder.1.bias": (16,),
                            "pe_encoder.2.weight": (8, 16), "pe_encoder.2.bias": (8,)}
    assert isinstance(enc.raw_norm, BatchNorm1d) and not hasattr(enc, "linear_x")


def test_encoder_refuses_a_batch_without_statistics():
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.data import Batch
    from graph_hscn.encoder import RWSENodeEncoder
    from graph_hscn.loader.synthetic import make_dataset
    enc = RWSENodeEncoder(RWSEConfig(9, 16, 8), 9, 16)
    with pytest.raises(ValueError, match="compute_rwse_stats_device"):
        enc(Batch.from_data_list(make_dataset("pcqm_contact", 2, seed=0)))


def test_device_statistics_refuse_cpu_tensors():
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.transform import compute_rwse_stats_device
    cfg = RWSEConfig(9, 16, 8, ksteps=4)
    graphs = make_dataset("pcqm_contact", 2, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_rwse_stats_device(Batch.from_data_list(graphs), True, cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_rwse_stats_device(graphs, True, cfg, device="cpu")
    assert not hasattr(graphs[0], "rwse")


def test_device_statistics_refuse_a_batch_outside_the_envelope_before_any_launch():
    """The envelope check reads host numbers only; it names both (CPU tensors would raise a different text after it
    if it were passed, so the order is visible here)."""
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.data import Batch
    from graph_hscn.transform.rwse import _rwse_launch

    class _OnDevice:                                   # passes _hip.ptr's is_cuda / contiguity questions, never read
        is_cuda = True
        device = "cuda"

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 0

    b = Batch(edge_index=_OnDevice(), num_nodes=600)
    b.ptr32, b.max_nodes, b.num_graphs = torch.tensor([0, 600], dtype=torch.int32), 600, 1
    with pytest.raises(RuntimeError, match=r"600 nodes.*ksteps is 20"):
        _rwse_launch(b, True, RWSEConfig(9, 16, 8))
    b.max_nodes = 100
    with pytest.raises(RuntimeError, match=r"100 nodes.*ksteps is 65"):
        _rwse_launch(b, True, RWSEConfig(9, 16, 8, ksteps=65))
