"""PNAConv without a GPU: parameter names and shapes, the config records, every refusal by name, the C entry points'
argument checks (before any launch), and the properties of the restatement the GPU tests hold the kernels to."""
import ctypes

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import (ACT_DICT, CONV_DICT, EDGE_AWARE_CONVS, GPSConfig, MPNNConfig, PNAConfig)
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.model.hscn import build_conv_relation
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import PNA, PNAConv, PNAEdge, pna_avg_deg_log
from graph_hscn.nn.gps import LOCAL_CONVS, GPSLayer
from tests import pna_oracle as PO

BADARG, UNSUPPORTED = -1, -3


# --------------------------------------------------------------------------- #
# the layer
# --------------------------------------------------------------------------- #
def test_state_dict_keys_and_shapes_are_pygs():
    c = PNAConv(12, 20, ("mean", "min", "max", "std"), ("identity", "amplification", "attenuation"), deg=torch.tensor([0, 3, 5, 2]),
                edge_dim=7)
    shapes = {k: tuple(v.shape) for k, v in c.state_dict().items()}
    assert shapes == {"edge_encoder.weight": (12, 7), "edge_encoder.bias": (12,),
                      "pre_nns.0.0.weight": (12, 36), "pre_nns.0.0.bias": (12,),
                      "post_nns.0.0.weight": (20, (3 * 4 + 1) * 12), "post_nns.0.0.bias": (20,),
                      "lin.weight": (20, 20), "lin.bias": (20,)}
    c = PNAConv(12, 20, ("sum",), ("identity",))
    shapes = {k: tuple(v.shape) for k, v in c.state_dict().items()}
    assert shapes == {"pre_nns.0.0.weight": (12, 24), "pre_nns.0.0.bias": (12,), "post_nns.0.0.weight": (20, 24),
                      "post_nns.0.0.bias": (20,), "lin.weight": (20, 20), "lin.bias": (20,)}
    assert sorted(PNA(8, 8).state_dict()) == sorted(k for k in PNAEdge(8, 8, edge_dim=3).state_dict() if "edge_encoder" not in k)
    assert PNAEdge.uses_edge_attr and not getattr(PNA, "uses_edge_attr", False)


def test_avg_deg_log_from_the_histogram_and_from_graphs():
    import math
    hist = torch.tensor([2, 0, 5, 1])                   # two nodes of in-degree 0, five of 2, one of 3
    want = (2 * math.log(1) + 5 * math.log(3) + math.log(4)) / 8
    assert abs(pna_avg_deg_log(hist) - want) < 1e-15
    c = PNAConv(4, 4, ("mean",), ("amplification",), deg=hist)
    assert abs(c.avg_deg_log - want) < 1e-15
    assert PNAConv(4, 4, ("mean",), ("attenuation",), avg_deg_log=0.5).avg_deg_log == 0.5
    assert PNAConv(4, 4, ("mean",), ("identity",)).avg_deg_log is None       # not needed, not asked for

    class G:
        num_nodes = 5
        edge_index = torch.tensor([[0, 1, 2, 0], [1, 1, 1, 3]])             # in-degrees 0, 3, 0, 1, 0
    want = (math.log(4) + math.log(2)) / 5
    assert abs(PNAConfig.avg_deg_log_of([G]) - want) < 1e-15
    cfg = PNAConfig.from_graphs([G, G])
    assert abs(cfg.avg_deg_log - want) < 1e-15 and cfg.scalers == ("identity", "amplification", "attenuation")
    with pytest.raises(ValueError, match="histogram"):
        pna_avg_deg_log(torch.zeros(3))


def test_every_refusal_by_name():
    ok = dict(aggregators=("mean",), scalers=("identity",))
    for kw, word in ((dict(towers=2), "towers"), (dict(pre_layers=2), "pre_layers"), (dict(post_layers=2), "post_layers"),
                     (dict(divide_input=True), "divide_input"), (dict(train_norm=True), "train_norm")):
        with pytest.raises(NotImplementedError, match=word):
            PNAConv(8, 8, **ok, **kw)
    for s in ("linear", "inverse_linear"):
        with pytest.raises(NotImplementedError, match=s):
            PNAConv(8, 8, ("mean",), ("identity", s), avg_deg_log=1.0)
    with pytest.raises(ValueError, match="unknown"):
        PNAConv(8, 8, ("median",), ("identity",))
    with pytest.raises(ValueError, match="at least one"):
        PNAConv(8, 8, (), ("identity",))
    with pytest.raises(ValueError, match="repeats"):
        PNAConv(8, 8, ("max", "max"), ("identity",))
    with pytest.raises(ValueError, match="avg_deg_log"):
        PNAConv(8, 8, ("mean",), ("amplification",))
    with pytest.raises(ValueError, match="positive"):
        PNAConv(8, 8, ("mean",), ("amplification",), avg_deg_log=0.0)
    with pytest.raises(ValueError, match="envelope"):
        PNAConv(513, 8, **ok)
    c = PNAConv(8, 8, **ok)
    x, ei = torch.zeros(4, 8), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="without edge_dim"):
        c(x, ei, torch.zeros(3, 2))
    with pytest.raises(ValueError, match="needs edge_attr"):
        PNAConv(8, 8, edge_dim=2, **ok)(x, ei)
    with pytest.raises(ValueError, match=r"\[N, 8\]"):
        c(torch.zeros(4, 9), ei)
    with pytest.raises(ValueError, match="HSCN's relations do not take"):
        build_conv_relation("PNA", 16)


# --------------------------------------------------------------------------- #
# config and models
# --------------------------------------------------------------------------- #
def test_registry_only_gained_entries():
    assert CONV_DICT["pna"] is PNA and CONV_DICT["pna_edge"] is PNAEdge
    assert list(CONV_DICT)[:6] == ["gcn", "gat", "gine", "gatedgcn", "transformerconv", "transformerconv_edge"]
    assert EDGE_AWARE_CONVS[:3] == ("gine", "gatedgcn", "transformerconv_edge") and "pna_edge" in EDGE_AWARE_CONVS
    assert "pna" not in EDGE_AWARE_CONVS
    assert LOCAL_CONVS[:6] == ("gcn", "gat", "gine", "gatedgcn", "transformerconv", "transformerconv_edge")
    assert {"pna", "pna_edge"} <= set(LOCAL_CONVS)


def test_pna_config_validates_its_fields():
    d = PNAConfig()
    assert d.aggregators == ("mean", "min", "max", "std") and d.scalers == ("identity",) and d.avg_deg_log is None
    assert PNAConfig(["sum", "std"], ["attenuation"], 1.5).aggregators == ("sum", "std")
    for kw in (dict(aggregators=()), dict(aggregators=("mean", "mean")), dict(aggregators=("mode",)), dict(aggregators="mean"),
               dict(scalers=()), dict(scalers=("linear",), avg_deg_log=1.0), dict(scalers=("amplification",)),
               dict(avg_deg_log=0.0), dict(avg_deg_log=float("inf")), dict(avg_deg_log="1")):
        with pytest.raises(ValueError):
            PNAConfig(**kw)


def test_model_configs_take_pna_last_and_check_it():
    import dataclasses
    assert [f.name for f in dataclasses.fields(MPNNConfig)][-1] == "pna"
    assert [f.name for f in dataclasses.fields(GPSConfig)][-1] == "pna"
    assert MPNNConfig("gcn", "relu").pna is None and GPSConfig("relu").pna is None
    cfg = PNAConfig(("mean", "max"), ("identity", "amplification"), 1.2)
    assert MPNNConfig("pna", "relu", pna=cfg).pna is cfg and GPSConfig("relu", "pna_edge", pna=cfg).pna is cfg
    with pytest.raises(ValueError, match="PNA convolution"):
        MPNNConfig("gcn", "relu", pna=cfg)
    with pytest.raises(ValueError, match="PNA convolution"):
        GPSConfig("relu", "gine", pna=cfg)
    with pytest.raises(ValueError, match="PNAConfig"):
        MPNNConfig("pna", "relu", pna={"aggregators": ("mean",)})
    MPNNConfig("pna_edge", "relu", edge_encoder="bond")
    with pytest.raises(ValueError, match="edge-aware"):
        MPNNConfig("pna", "relu", edge_encoder="bond")


def test_models_build_their_layers_from_the_config():
    cfg = PNAConfig(("mean", "max"), ("identity", "amplification"), 1.2)
    m = build_mpnn(MPNNConfig("pna_edge", "relu", hidden_channels=16, num_layers=3, pna=cfg), 9, 10)
    assert [type(c) for c in m.conv_layers] == [PNAEdge] * 3 and m.layered_only
    assert all(c.aggregators == cfg.aggregators and c.scalers == cfg.scalers and c.avg_deg_log == 1.2 for c in m.conv_layers)
    assert tuple(m.conv_layers[0].post_nns[0][0].weight.shape) == (16, 5 * 9)
    assert m.resident_reason().startswith("convolution PNAConv")
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="convolution PNAConv"):
        m._forward(None)
    d = build_mpnn(MPNNConfig("pna", "relu"), 9, 10)
    assert [type(c) for c in d.conv_layers] == [PNA] * 3 and d.conv_layers[0].aggregators == ("mean", "min", "max", "std")
    g = build_gps(GPSConfig("relu", "pna_edge", hidden_channels=16, num_layers=2, edge_encoder="bond", pna=cfg), 9, 10)
    assert all(isinstance(layer.conv, PNAEdge) and layer.conv.scalers == cfg.scalers for layer in g.layers)
    assert g.layers[0].uses_edge_attr and not g.layers[0].updates_edge_attr and hasattr(g, "edge_encoder")
    assert isinstance(GPS(9, 16, 10, 1, local_conv="pna").layers[0].conv, PNA)
    with pytest.raises(ValueError, match="pna_edge"):
        GPSLayer(16, "gcn", 4, pna=cfg)
    with pytest.raises(ValueError, match="PNA convolution"):
        MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 10, 3, pna=cfg)
    with pytest.raises(ValueError, match="edge-aware"):
        MPNN(CONV_DICT["pna"], ACT_DICT["relu"], 9, 16, 10, 3, edge_encoder="bond")

    class B:
        x = torch.zeros(3, 9)
        edge_index = torch.zeros(2, 0, dtype=torch.int64)
        batch = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="'pna_edge'"):
        m.engine = "layered"
        m._forward(B)


# --------------------------------------------------------------------------- #
# the C entry points: refusals before any launch
# --------------------------------------------------------------------------- #
_BUF = ctypes.create_string_buffer(64)
_HERE = ctypes.addressof(_BUF)


def _codes(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _fwd(lib, F, aggr=(0, 1, 2, 3, 4), scal=(0, 1, 2), avg=1.0, N=0, E=0, ptrs=None, aggr_n=None, scal_n=None):
    p = ptrs if ptrs is not None else [None] * 10
    return lib.hscn_pna_fwd(*p, N, E, F, _codes(*aggr) if aggr is not None else None, len(aggr) if aggr_n is None else aggr_n,
                            _codes(*scal) if scal is not None else None, len(scal) if scal_n is None else scal_n, avg,
                            None, None)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _hip.lib()
    assert Fh.PNA_LONG_ROW == lib.hscn_pna_long_row() == lib.hscn_gine_long_row()
    assert Fh.PNA_CHUNK == lib.hscn_pna_chunk() == lib.hscn_gine_chunk()
    # the envelope: hscn_pna_supported is what the Python layers ask
    assert [lib.hscn_pna_supported(F, 5, 3) for F in (0, 1, 512, 513)] == [0, 1, 1, 0]
    assert lib.hscn_pna_supported(16, 0, 1) == 0 and lib.hscn_pna_supported(16, 6, 1) == 0
    assert lib.hscn_pna_supported(16, 1, 0) == 0 and lib.hscn_pna_supported(16, 1, 4) == 0
    assert Fh.pna_supported(Fh.PNA_MAX_WIDTH, 5, 3) and not Fh.pna_supported(Fh.PNA_MAX_WIDTH + 1, 5, 3)
    # F = 0: bad argument; 512: inside (N = 0: nothing to do; N > 0 over NULL pointers: bad argument); 513: unsupported
    assert _fwd(lib, 0) == BADARG and _fwd(lib, 512) == 0 and _fwd(lib, 513) == UNSUPPORTED
    assert _fwd(lib, 512, N=4) == BADARG and _fwd(lib, 513, N=4) == UNSUPPORTED and _fwd(lib, 0, N=4) == BADARG
    assert _fwd(lib, 16, N=-1) == BADARG and _fwd(lib, 16, E=-1) == BADARG and _fwd(lib, 16, N=1 << 31) == BADARG
    # the lists: empty, too long, an unknown code, a repeat, a NULL list
    for kw in (dict(aggr=()), dict(aggr=(0, 1, 2, 3, 4), aggr_n=6), dict(aggr=(5,)), dict(aggr=(-1,)), dict(aggr=(2, 2)),
               dict(aggr=None, aggr_n=1), dict(scal=()), dict(scal=(3,)), dict(scal=(1, 1)), dict(scal=None, scal_n=1),
               dict(scal=(0, 1, 2), scal_n=4)):
        assert _fwd(lib, 16, **kw) == BADARG, kw
    # avg_deg_log is read beside a degree scaler only
    for avg in (0.0, -1.0, float("nan"), float("inf")):
        assert _fwd(lib, 16, scal=(0,), avg=avg) == 0
        assert _fwd(lib, 16, scal=(0, 2), avg=avg) == BADARG and _fwd(lib, 16, scal=(1,), avg=avg) == BADARG
    # every required pointer: all given but one
    full = [_HERE] * 7 + [None, None, None]
    for missing in (0, 3, 4, 6):
        p = list(full)
        p[missing] = None
        assert _fwd(lib, 16, N=4, ptrs=p) == BADARG, missing
    assert _fwd(lib, 16, N=4, ptrs=full) == BADARG                                     # (flag is NULL)
    ag, sc = _codes(0, 4), _codes(0)
    assert lib.hscn_pna_bwd_fold(None, None, None, None, None, 4, 0, ag, 2, sc, 1, 0.0, None) == BADARG
    assert lib.hscn_pna_bwd_fold(None, None, None, None, None, 4, 513, ag, 2, sc, 1, 0.0, None) == UNSUPPORTED
    assert lib.hscn_pna_bwd_fold(None, None, None, None, None, 0, 512, ag, 2, sc, 1, 0.0, None) == 0
    assert lib.hscn_pna_bwd_fold(None, None, None, None, None, 4, 512, ag, 2, sc, 1, 0.0, None) == BADARG
    assert lib.hscn_pna_bwd_fold(_HERE, _HERE, None, _HERE, None, 4, 16, ag, 2, sc, 1, 0.0, None) == BADARG   # std needs stdv
    for name, lead in (("hscn_pna_bwd_src", 9), ("hscn_pna_bwd_edge", 7)):
        fn = getattr(lib, name)
        assert fn(*[None] * lead, 4, 4, 0, None, None) == BADARG
        assert fn(*[None] * lead, 4, 4, 513, None, None) == UNSUPPORTED
        assert fn(*[None] * lead, 4, 4, 512, None, None) == BADARG
        assert fn(*[None] * lead, -1, 4, 16, None, None) == BADARG
        assert fn(*[None] * lead, 0, 0, 512, None, None) == 0


def test_operand_checks_that_need_no_device():
    class Rel:
        num_src = num_dst = 4
        num_edges = 3
        _csr_t = None
    a = torch.zeros(4, 8)
    with pytest.raises(TypeError, match="float32"):
        Fh.PNAAggregateFn.apply(a.double(), a, None, Rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="contiguous"):
        Fh.PNAAggregateFn.apply(a, torch.zeros(8, 4).t(), None, Rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="b is"):
        Fh.PNAAggregateFn.apply(a, torch.zeros(4, 7), None, Rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="rows"):
        Fh.PNAAggregateFn.apply(torch.zeros(5, 8), torch.zeros(5, 8), None, Rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="3 edges"):
        Fh.PNAAggregateFn.apply(a, a, torch.zeros(2, 8), Rel, ("max",), ("identity",))
    with pytest.raises(ValueError, match="unknown"):
        Fh.PNAAggregateFn.apply(a, a, None, Rel, ("maximum",), ("identity",))
    with pytest.raises(ValueError, match="avg_deg_log"):
        Fh.PNAAggregateFn.apply(a, a, None, Rel, ("max",), ("attenuation",), None)
    with pytest.raises(RuntimeError, match="CPU"):
        Fh.PNAAggregateFn.apply(a, a, None, Rel, ("max",), ("identity",))


# --------------------------------------------------------------------------- #
# the restatement's own properties
# --------------------------------------------------------------------------- #
def test_oracle_gives_an_empty_row_zeros_and_the_std_floor():
    a = torch.randn(3, 2, dtype=torch.float64)
    b = torch.randn(3, 2, dtype=torch.float64)
    ei = torch.tensor([[0, 1], [0, 0]])                                     # nodes 1 and 2 have no in-edge
    out = PO.aggregate(a, b, None, ei, PO.AGGREGATORS, PO.SCALERS, 0.7).view(3, 3, 5, 2)
    assert bool((out[1:, :, :4] == 0).all())
    d1 = torch.log(torch.tensor(2.0, dtype=torch.float64))
    for s, scale in enumerate((1.0, d1 / 0.7, 0.7 / d1)):                   # the scalers see d = max(deg, 1) = 1
        assert torch.allclose(out[1:, s, 4], torch.full((2, 2), 1e-5, dtype=torch.float64).sqrt() * scale, rtol=1e-15)
    m = a[0] + b[:2]                                                        # node 0: two messages
    assert torch.allclose(out[0, 0, 0], m.mean(0)) and torch.allclose(out[0, 0, 3], m.sum(0))
    assert torch.equal(out[0, 0, 1], m.min(0).values) and torch.equal(out[0, 0, 2], m.max(0).values)
    assert torch.allclose(out[0, 0, 4], (m.var(0, unbiased=False) + 1e-5).sqrt())
    d2 = torch.log(torch.tensor(3.0, dtype=torch.float64))
    assert torch.allclose(out[0, 1], out[0, 0] * d2 / 0.7) and torch.allclose(out[0, 2], out[0, 0] * 0.7 / d2)


def test_oracle_sends_a_tie_to_the_first_edge():
    # three edges into node 0; column 0: edges 0 and 2 tie for the max, column 1: edges 1 and 2 tie for the min
    a = torch.zeros(4, 2, dtype=torch.float64)
    b = torch.tensor([[0., 0.], [5., 3.], [1., 1.], [5., 1.]], dtype=torch.float64, requires_grad=True)
    ei = torch.tensor([[1, 2, 3], [0, 0, 0]])
    t = torch.zeros(3, 2, dtype=torch.float64, requires_grad=True)
    out = PO.aggregate(a, b, t, ei, ("max", "min"), ("identity",))
    assert out[0].tolist() == [5.0, 3.0, 1.0, 1.0]
    out[0].backward(torch.tensor([1.0, 10.0, 100.0, 1000.0], dtype=torch.float64))
    # max: column 0 -> edge 0 (first of the tie), column 1 -> edge 0; min: column 0 -> edge 1, column 1 -> edge 1 (first)
    assert t.grad.tolist() == [[1.0, 10.0], [100.0, 1000.0], [0.0, 0.0]]
    assert b.grad.tolist() == [[0.0, 0.0], [1.0, 10.0], [100.0, 1000.0], [0.0, 0.0]]
    # the edge list reordered: the tie follows the order of the list, not the source's number
    t2 = torch.zeros(3, 2, dtype=torch.float64, requires_grad=True)
    PO.aggregate(a, b.detach(), t2, ei[:, [2, 1, 0]], ("max",), ("identity",))[0].backward(torch.ones(2, dtype=torch.float64))
    assert t2.grad.tolist() == [[1.0, 0.0], [0.0, 0.0], [0.0, 1.0]]
    # std of a repeated message: variance exactly 0, no gradient through the relu
    b3 = torch.tensor([[0.3, -0.7]], dtype=torch.float32, requires_grad=True)
    out = PO.aggregate(torch.zeros(1, 2), b3, None, torch.tensor([[0, 0], [0, 0]]), ("std",), ("identity",))
    assert torch.equal(out, torch.full((1, 2), 1e-5).sqrt())
    out.sum().backward()
    assert bool((b3.grad == 0).all())
