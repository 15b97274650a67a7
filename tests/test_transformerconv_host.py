"""TransformerConv without a GPU: the restatement of tests/transformerconv_oracle.py against an independent dense
formulation, the module's surface (PyG's parameters and ``state_dict`` keys), the registry and config validation, the
refusals by name, and the binding of the hscn_edge_attn_* entry points (envelope, constants, argument checks before any
launch)."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import (ACT_DICT, CONV_DICT, EDGE_AWARE_CONVS, GPSConfig, HSCNConfig, MPNNConfig)
from graph_hscn.model.gps import build_gps
from graph_hscn.model.hscn import HSCN, build_conv_relation, build_hscn
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import EdgeTransformerConv, GATConv, TransformerConv
from tests import transformerconv_oracle as TO


# ---- the oracle against a dense restatement ------------------------------------------------------------------------
def _multigraph(N, E, seed):
    """tests/test_gpu_gine.py's shape: random edge order, the last four nodes isolated, two self loops, two edges
    occurring three times."""
    g = torch.Generator().manual_seed(seed)
    live = max(N - 4, 1)
    base = torch.randint(0, live, (2, E - 6), generator=g)
    extra = torch.tensor([[1 % live, 2 % live], [1 % live, 2 % live]])
    ei = torch.cat([base, extra, base[:, :2], base[:, :2]], 1)
    return ei[:, torch.randperm(E, generator=g)].contiguous()


@pytest.mark.parametrize("heads,C", [(1, 10), (2, 8), (3, 5), (4, 4)])
def test_the_oracle_agrees_with_the_dense_multiplicity_form(heads, C):
    """Both sides float64, differing by summation order only: 1e-12."""
    ei = _multigraph(37, 150, 3)
    g = torch.Generator().manual_seed(heads * 100 + C)
    q, k, v = (torch.randn(37, heads * C, generator=g, dtype=torch.float64) for _ in range(3))
    a, d = TO.aggregate(q, k, v, None, ei, heads), TO.dense(q, k, v, ei, heads)
    assert float((a - d).abs().max()) <= 1e-12
    assert bool((a[-4:] == 0).all())                       # the isolated nodes
    # bipartite, 50 -> 4
    src, dst = torch.randint(0, 50, (200,), generator=g), torch.randint(0, 4, (200,), generator=g)
    ei = torch.stack([src, dst])
    q = torch.randn(4, heads * C, generator=g, dtype=torch.float64)
    k, v = (torch.randn(50, heads * C, generator=g, dtype=torch.float64) for _ in range(2))
    assert float((TO.aggregate(q, k, v, None, ei, heads) - TO.dense(q, k, v, ei, heads)).abs().max()) <= 1e-12


def test_the_oracle_with_edge_features_equals_the_plain_one_on_shifted_keys_and_values():
    """One in-edge per target: the weight is 1 and ``out = v[j] + e`` exactly; and ``skip`` removes exactly one edge."""
    g = torch.Generator().manual_seed(0)
    ei = torch.stack([torch.randint(0, 4, (50,), generator=g), torch.arange(50)])
    q = torch.randn(50, 8, generator=g, dtype=torch.float64)
    k, v = torch.randn(4, 8, generator=g, dtype=torch.float64), torch.randn(4, 8, generator=g, dtype=torch.float64)
    e = torch.randn(50, 8, generator=g, dtype=torch.float64)
    assert torch.equal(TO.aggregate(q, k, v, e, ei, 2), v[ei[0]] + e)
    ei = _multigraph(37, 150, 1)
    q, k, v = (torch.randn(37, 8, generator=g, dtype=torch.float64) for _ in range(3))
    e = torch.randn(150, 8, generator=g, dtype=torch.float64)
    keep = torch.ones(150, dtype=torch.bool)
    keep[17] = False
    assert torch.equal(TO.aggregate(q, k, v, e, ei, 2, skip=17), TO.aggregate(q, k, v, e[keep], ei[:, keep], 2))


# ---- module surface --------------------------------------------------------------------------------------------------
def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_state_dict_keys_and_shapes_are_pygs():
    m = TransformerConv(9, 4, heads=3)
    assert _shapes(m) == {"lin_key.weight": (12, 9), "lin_key.bias": (12,), "lin_query.weight": (12, 9),
                          "lin_query.bias": (12,), "lin_value.weight": (12, 9), "lin_value.bias": (12,),
                          "lin_skip.weight": (12, 9), "lin_skip.bias": (12,)}
    assert sum(p.numel() for p in m.parameters()) == 4 * (12 * 9 + 12)
    m = TransformerConv((9, 5), 4, heads=3, edge_dim=7, bias=False)
    assert _shapes(m) == {"lin_key.weight": (12, 9), "lin_key.bias": (12,), "lin_query.weight": (12, 5),
                          "lin_query.bias": (12,), "lin_value.weight": (12, 9), "lin_value.bias": (12,),
                          "lin_edge.weight": (12, 7), "lin_skip.weight": (12, 5)}
    m = TransformerConv(9, 4, heads=2, root_weight=False)
    assert sorted(_shapes(m)) == ["lin_key.bias", "lin_key.weight", "lin_query.bias", "lin_query.weight",
                                  "lin_value.bias", "lin_value.weight"]
    # the same keys as the restatement, so a state_dict moves across
    assert sorted(TO.TransformerConvRef((9, 5), 4, 3, edge_dim=7).state_dict()) == \
        sorted(TransformerConv((9, 5), 4, heads=3, edge_dim=7).state_dict())
    # lazy widths: the weights exist, unmaterialised, under the same keys
    lazy = TransformerConv(-1, 4, heads=2, edge_dim=-1)
    assert sorted(lazy.state_dict()) == sorted(TransformerConv(3, 4, heads=2, edge_dim=5).state_dict())
    assert isinstance(lazy.lin_key.weight, torch.nn.parameter.UninitializedParameter)
    assert isinstance(lazy.lin_edge.weight, torch.nn.parameter.UninitializedParameter)
    e = EdgeTransformerConv(9, 4, heads=2)
    assert e.uses_edge_attr and e.lin_edge is not None and e.lin_edge.bias is None and e.heads == 2
    assert not getattr(TransformerConv, "uses_edge_attr", False)


def test_what_is_not_provided_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="concat=False"):
        TransformerConv(9, 4, concat=False)
    with pytest.raises(NotImplementedError, match="beta=True"):
        TransformerConv(9, 4, beta=True)
    with pytest.raises(NotImplementedError, match="dropout"):
        TransformerConv(9, 4, dropout=0.1)
    with pytest.raises(ValueError, match="envelope"):
        TransformerConv(9, 65, heads=8)
    with pytest.raises(NotImplementedError):               # pinned by tests/test_gat_self_loops_host.py, still refused
        GATConv(3, 4, heads=2)


def test_registry_and_configs():
    assert CONV_DICT["transformerconv"] is TransformerConv and CONV_DICT["transformerconv_edge"] is EdgeTransformerConv
    assert "transformer" not in CONV_DICT and "transformerconv_edge" in EDGE_AWARE_CONVS
    assert "transformerconv" not in EDGE_AWARE_CONVS
    with pytest.raises(ValueError):                        # pinned by tests/test_attention_host.py, still refused
        GPSConfig("relu", local_conv_type="transformer")
    assert MPNNConfig("gcn", "relu").heads == 1
    assert MPNNConfig("transformerconv", "relu", heads=4).heads == 4
    with pytest.raises(ValueError, match="divisible"):
        MPNNConfig("transformerconv", "relu", hidden_channels=16, heads=3)
    with pytest.raises(ValueError, match="heads=2"):
        MPNNConfig("gcn", "relu", heads=2)
    with pytest.raises(ValueError, match="heads"):
        MPNNConfig("transformerconv", "relu", heads=0)
    with pytest.raises(ValueError, match="edge-aware"):
        MPNNConfig("transformerconv", "relu", edge_encoder="bond")
    assert MPNNConfig("transformerconv_edge", "relu", edge_encoder="bond", heads=2).edge_encoder == "bond"
    assert HSCNConfig("relu").heads == 1
    assert HSCNConfig("relu", "TransformerConv", heads=2).heads == 2
    with pytest.raises(ValueError, match="TransformerConv"):
        HSCNConfig("relu", heads=2)
    with pytest.raises(ValueError, match="divisible"):
        HSCNConfig("relu", "TransformerConv", hidden_channels=16, heads=3)
    with pytest.raises(TypeError):                         # keyword-only: the positional order is what it was
        HSCNConfig("relu", "GAT", "GCN", "GCN", 16, 3, 4, 10, [16], None, 2)


def test_models_are_built_with_heads_and_are_layered_only():
    m = build_mpnn(MPNNConfig("transformerconv", "relu", hidden_channels=16, num_layers=3, heads=4), 9, 10)
    assert [(c.heads, c.out_channels) for c in m.conv_layers] == [(4, 4), (4, 4), (1, 10)]
    assert m.conv_layers[0].lin_key.weight.shape == (16, 9) and m.conv_layers[2].lin_key.weight.shape == (10, 16)
    assert m.resident_reason().startswith("convolution TransformerConv") and m.layered_only and not m.supported()
    for level in ("node", "link"):
        lm = MPNN(TransformerConv, ACT_DICT["relu"], 9, 16, 10, 3, task_level=level, heads=2)
        assert lm.resident_reason().startswith("convolution TransformerConv")
    e = build_mpnn(MPNNConfig("transformerconv_edge", "relu", edge_encoder="bond", heads=2), 9, 10)
    assert all(isinstance(c, EdgeTransformerConv) and c.lin_edge is not None for c in e.conv_layers)
    assert e.resident_reason().startswith("convolution EdgeTransformerConv")
    with pytest.raises(ValueError, match="heads=2"):
        MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 10, 3, heads=2)
    with pytest.raises(ValueError, match="divisible"):
        MPNN(TransformerConv, ACT_DICT["relu"], 9, 16, 10, 3, heads=3)
    with pytest.raises(ValueError, match="edge-aware"):
        MPNN(TransformerConv, ACT_DICT["relu"], 9, 16, 10, 3, edge_encoder="bond")
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        m(SimpleNamespace())
    # the refusals every resident, captured and one-launch entry point goes through
    from graph_hscn.train import batching
    with pytest.raises(RuntimeError, match="convolution TransformerConv"):
        batching.refuse_layered_only(m, "the one-launch MPNN step")

    g = build_gps(GPSConfig("relu", local_conv_type="transformerconv_edge", hidden_channels=16, num_heads=4), 9, 10)
    assert all(isinstance(l.conv, EdgeTransformerConv) and (l.conv.heads, l.conv.out_channels) == (4, 4) for l in g.layers)
    assert g.layers[0].uses_edge_attr and not g.layers[0].updates_edge_attr and g.resident_reason() is not None
    g = build_gps(GPSConfig("relu", local_conv_type="transformerconv", hidden_channels=16, num_heads=2), 9, 10)
    assert type(g.layers[0].conv) is TransformerConv and g.layers[0].conv.lin_key.weight.shape == (16, 16)

    h = build_hscn(HSCNConfig("relu", "TransformerConv", "TransformerConv", "TransformerConv", hidden_channels=16,
                              num_layers=2, heads=2), 9, 10)
    for conv in h.convs:
        assert all(type(c) is TransformerConv and (c.heads, c.out_channels) == (2, 8) for c in conv.convs.values())
    assert h.convs[0].convs["local__to__virtual"].lin_key.weight.shape == (16, 9)
    assert h.resident_reason() is not None and h._resident_params() is None
    mixed = HSCN("GAT", "TransformerConv", "GCN", ACT_DICT["relu"], 9, 16, 10, 2, heads=4)
    assert type(mixed.convs[0].convs["local__to__local"]) is TransformerConv
    assert isinstance(mixed.convs[0].convs["local__to__virtual"], GATConv)
    with pytest.raises(ValueError, match="TransformerConv"):
        HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 2, heads=2)
    with pytest.raises(ValueError, match="vl_conv"):       # the pinned refusal: vl_conv stays None or "GAT"
        HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 2, vl_conv="TransformerConv")


def test_build_conv_relation():
    c = build_conv_relation("TransformerConv", 16, 9, heads=4)
    assert type(c) is TransformerConv and (c.heads, c.out_channels, c.in_channels) == (4, 4, (9, 9))
    lazy = build_conv_relation("TransformerConv", 16)
    assert isinstance(lazy.lin_query.weight, torch.nn.parameter.UninitializedParameter)
    with pytest.raises(ValueError, match="edge features"):
        build_conv_relation("TransformerConv_edge", 16)
    with pytest.raises(ValueError, match="edge features"):  # the same kind of refusal as
        build_conv_relation("GINE", 16)
    with pytest.raises(ValueError, match="divisible"):
        build_conv_relation("TransformerConv", 16, 9, heads=3)
    with pytest.raises(ValueError, match="heads=2"):
        build_conv_relation("GCN", 16, 9, heads=2)


# ---- binding ---------------------------------------------------------------------------------------------------------
NEW = ("hscn_edge_attn_supported", "hscn_edge_attn_long_row", "hscn_edge_attn_chunk", "hscn_edge_attn_fwd",
       "hscn_edge_attn_bwd_dst", "hscn_edge_attn_bwd_src")


def test_the_binding_exports_the_new_symbols_under_the_same_abi():
    lib = _hip.lib()
    assert set(NEW) <= set(_hip.exported_symbols())
    assert lib.hscn_abi_version() == 24 == _hip.ABI_VERSION
    for name in NEW:
        types = _hip._SIGNATURES[name][1]                  # none of them is a flagged entry point
        assert not (len(types) >= 2 and types[-2] is ctypes.c_int and types[-1] is ctypes.c_void_p), name


@pytest.mark.parametrize("heads,C,answer", [(1, 1, 1), (1, 10, 1), (8, 64, 1), (1, 512, 1), (8, 65, 0), (0, 4, 0),
                                            (1, 0, 0)])
def test_the_envelope_has_one_source(heads, C, answer):
    assert _hip.lib().hscn_edge_attn_supported(heads, C) == answer
    assert Fh.edge_attn_supported(heads, C) == bool(answer)


def test_constants_are_the_librarys():
    lib = _hip.lib()
    assert Fh.EDGE_ATTN_LONG_ROW == lib.hscn_edge_attn_long_row()
    assert Fh.EDGE_ATTN_CHUNK == lib.hscn_edge_attn_chunk()
    assert Fh.EDGE_ATTN_MAX_WIDTH == 512


def _blank(name, **at):
    types = _hip._SIGNATURES[name][1]
    args = [None if t is ctypes.c_void_p else 0 for t in types]
    for pos, v in at.items():
        args[int(pos[1:])] = v
    return getattr(_hip.lib(), name)(*args)


def test_null_pointers_and_negative_sizes_are_refused_before_any_launch():
    """No device is needed: the checks come before the first HIP call.  Positions: fwd Nd, Ns, E, heads, head_dim =
    9..13; bwd_dst 13..17; bwd_src 12..16."""
    for name, first in (("hscn_edge_attn_fwd", 9), ("hscn_edge_attn_bwd_dst", 13), ("hscn_edge_attn_bwd_src", 12)):
        ok = {f"p{first}": 3, f"p{first + 1}": 3, f"p{first + 2}": 2, f"p{first + 3}": 2, f"p{first + 4}": 4}
        assert _blank(name, **ok) == -1, name                                     # every pointer NULL
        for k in range(3):
            assert _blank(name, **{**ok, f"p{first + k}": -1}) == -1, (name, k)   # a negative size
        assert _blank(name, **{**ok, f"p{first + 3}": 0}) == -1, name             # no heads
        assert _blank(name, **{**ok, f"p{first + 3}": 8, f"p{first + 4}": 65}) == -3, name     # HSCN_E_UNSUPPORTED


# ---- no GPU: refusals by name ----------------------------------------------------------------------------------------
def _rel(num_src, num_dst, E):
    return SimpleNamespace(num_src=num_src, num_dst=num_dst, num_edges=E)


def test_the_function_checks_by_name_before_any_launch():
    q, k = torch.zeros(5, 8), torch.zeros(7, 8)
    apply = Fh.EdgeAttentionFn.apply
    with pytest.raises(TypeError, match="float32"):
        apply(q.double(), k, k, None, _rel(7, 5, 3), 2)
    with pytest.raises(TypeError, match="float32"):
        apply(q, k, k, torch.zeros(3, 8, dtype=torch.int64), _rel(7, 5, 3), 2)
    with pytest.raises(ValueError, match="multiple of heads"):
        apply(q, k, k, None, _rel(7, 5, 3), 3)
    with pytest.raises(ValueError, match="k is"):
        apply(q, k, torch.zeros(7, 4), None, _rel(7, 5, 3), 2)
    with pytest.raises(ValueError, match="relation is"):
        apply(q, k, k, None, _rel(5, 7, 3), 2)
    with pytest.raises(ValueError, match="3 edges"):
        apply(q, k, k, torch.zeros(4, 8), _rel(7, 5, 3), 2)
    with pytest.raises(ValueError, match="envelope"):
        apply(torch.zeros(5, 520), torch.zeros(7, 520), torch.zeros(7, 520), None, _rel(7, 5, 3), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        apply(q, k, k, None, _rel(7, 5, 3), 2)


def test_cpu_tensors_have_no_fallback():
    conv = TransformerConv(9, 4, heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.zeros(5, 9), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="edge_attr"):
        EdgeTransformerConv(9, 4)(torch.zeros(5, 9), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="without edge_dim"):
        conv(torch.zeros(5, 9), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(3, 2))
