"""Categorical encoders (encoder/categorical.py, nn.functional.CategoricalEmbedFn), everything that runs without a GPU:
the CPU branch against OGB's construction (a ModuleList of nn.Embedding summed in column order), the OGB state-dict
round trip, config validation, ``to_device``'s dtype rule, the default models' parameter names and the C ABI's names."""
import os
import re

import pytest
import torch
import torch.nn as nn

from graph_hscn import _hip
from graph_hscn.config.config import GPSConfig, MPNNConfig
from graph_hscn.data import Batch
from graph_hscn.encoder import (ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS, AtomEncoder, BondEncoder, CategoricalEncoder)
from graph_hscn.loader import synthetic
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import build_gps
from graph_hscn.model.mpnn import build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.train import batching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATENC_NAMES = ["hscn_catenc_bwd", "hscn_catenc_bwd_workspace_bytes", "hscn_catenc_chunk", "hscn_catenc_fwd",
                "hscn_catenc_index_build", "hscn_catenc_index_workspace_bytes", "hscn_catenc_long_row",
                "hscn_catenc_sort_chunk", "hscn_catenc_supported"]


def _categories(cards, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, c, (n,), generator=g) for c in cards], 1)


def _ogb_tables(enc, dtype=torch.float32):
    """OGB's encoder: one nn.Embedding per column, holding the encoder's blocks."""
    tables = nn.ModuleList(nn.Embedding(c, enc.emb_dim) for c in enc.cardinalities).to(dtype)
    tables.load_state_dict({k.split(".", 1)[1]: v.to(dtype) for k, v in enc.to_ogb_state_dict().items()})
    return tables


def test_feature_dims_are_the_loaders():
    assert list(ATOM_FEATURE_DIMS) == [int(c) for c in synthetic._ATOM_CARD]
    assert list(BOND_FEATURE_DIMS) == [int(c) for c in synthetic._BOND_CARD]
    assert AtomEncoder(16).weight.shape == (sum(ATOM_FEATURE_DIMS), 16)
    assert BondEncoder(8).weight.shape == (sum(BOND_FEATURE_DIMS), 8)


@pytest.mark.parametrize("make, n", [(lambda: AtomEncoder(16), 257), (lambda: BondEncoder(20), 64),
                                     (lambda: CategoricalEncoder([3], 4), 1), (lambda: AtomEncoder(8), 0)])
def test_cpu_branch_equals_a_module_list_of_embeddings(make, n):
    torch.manual_seed(3)
    enc = make()
    tables = _ogb_tables(enc)
    x = _categories(enc.cardinalities, n, 5)
    x[: min(n, 2)] = 0                                   # repeats of one category in every column
    out = enc(x)
    ref = 0
    for c, t in enumerate(tables):                       # OGB's loop
        ref = ref + t(x[:, c])
    assert out.shape == (n, enc.emb_dim) and torch.equal(out, ref)
    g = torch.randn(n, enc.emb_dim, generator=torch.Generator().manual_seed(7))
    out.backward(g)
    ref.backward(g)
    assert torch.equal(enc.weight.grad, torch.cat([t.weight.grad for t in tables]))
    # the Function's CPU branch is the restatement itself
    again = Fh.categorical_embed_reference(enc.weight, x, enc.cardinalities)
    assert torch.equal(again, out)


def test_each_column_block_is_initialised_by_itself():
    torch.manual_seed(0)
    enc = AtomEncoder(64)
    for c, card in enumerate(enc.cardinalities):         # xavier_uniform_ of a [card, D] table: |w| <= sqrt(6 / (card + D))
        block = enc.weight.detach()[enc.offsets[c]:enc.offsets[c + 1]]
        bound = (6.0 / (card + 64)) ** 0.5
        assert float(block.abs().max()) <= bound and float(block.abs().max()) > 0.5 * bound


def test_ogb_state_dict_round_trip_is_lossless():
    torch.manual_seed(1)
    a, b = AtomEncoder(12), AtomEncoder(12)
    state = a.to_ogb_state_dict()
    assert sorted(state) == sorted(f"atom_embedding_list.{c}.weight" for c in range(9))
    assert [tuple(state[f"atom_embedding_list.{c}.weight"].shape) for c in range(9)] == [(k, 12) for k in ATOM_FEATURE_DIMS]
    assert not torch.equal(a.weight, b.weight)
    b.load_ogb_state_dict(state)
    assert torch.equal(a.weight, b.weight)
    assert sorted(BondEncoder(4).to_ogb_state_dict()) == [f"bond_embedding_list.{c}.weight" for c in range(3)]
    with pytest.raises(KeyError):
        b.load_ogb_state_dict({k.replace("atom", "bond"): v for k, v in state.items()})
    bad = dict(state)
    bad["atom_embedding_list.0.weight"] = torch.zeros(118, 12)
    with pytest.raises(ValueError):
        b.load_ogb_state_dict(bad)
    assert torch.equal(a.weight, b.weight)               # a refused dict changes nothing
    # into OGB's own module layout
    tables = nn.ModuleList(nn.Embedding(c, 12) for c in ATOM_FEATURE_DIMS)
    tables.load_state_dict({k.split(".", 1)[1]: v for k, v in state.items()}, strict=True)


def test_construction_refuses_what_the_kernels_do_not_take():
    for cards, D in (([5, 6], 6), ([5, 6], 0), ([5, 6], 516), ([2] * 17, 16), ([4097], 16), ([], 16), ([3, 0], 16)):
        with pytest.raises(ValueError):
            CategoricalEncoder(cards, D)
    CategoricalEncoder([2] * 16, 512)
    CategoricalEncoder([4096], 4)
    # the host restatement of the envelope is the library's
    lib = _hip.lib()
    for D in (0, 3, 4, 6, 8, 20, 512, 516):
        for F in (0, 1, 9, 16, 17):
            for R in (0, 1, 8, 9, 16, 174, 4096, 4097):
                assert bool(lib.hscn_catenc_supported(D, F, R)) == Fh.catenc_supported(D, F, R), (D, F, R)


def test_inputs_that_are_not_categories_are_refused():
    enc = BondEncoder(8)
    with pytest.raises(TypeError, match="to_device"):
        enc(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        enc(torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(IndexError):                      # the CPU branch: torch's own bounds check
        enc(torch.tensor([[0, 6, 0]]))
    assert enc(torch.zeros(4, 3, dtype=torch.int32)).shape == (4, 8)
    wide = torch.zeros(4, 6, dtype=torch.int64)
    assert torch.equal(enc(wide[:, ::2]), enc(torch.zeros(4, 3, dtype=torch.int64)))     # non-contiguous: made contiguous


def test_config_validation():
    assert MPNNConfig("gcn", "relu").node_encoder is None and MPNNConfig("gcn", "relu").edge_encoder is None
    assert GPSConfig("relu").node_encoder is None and GPSConfig("relu").edge_encoder is None
    MPNNConfig("gcn", "relu", node_encoder="atom")
    MPNNConfig("gine", "relu", node_encoder="atom", edge_encoder="bond")
    GPSConfig("relu", local_conv_type="gatedgcn", node_encoder="atom", edge_encoder="bond")
    GPSConfig("relu", local_conv_type=None, node_encoder="atom")
    for bad in (dict(node_encoder="bond"), dict(node_encoder="Atom"), dict(edge_encoder="atom"), dict(edge_encoder="bond")):
        with pytest.raises(ValueError):
            MPNNConfig("gcn", "relu", **bad)             # ("bond" with gcn: no layer reads edge features)
    with pytest.raises(ValueError):
        GPSConfig("relu", local_conv_type=None, edge_encoder="bond")
    with pytest.raises(ValueError):
        GPSConfig("relu", local_conv_type="gat", edge_encoder="bond")
    # the trailing position: every earlier positional argument means what it meant
    assert MPNNConfig("gcn", "relu", 32, 4, 0.1, False, False, "node").task_level == "node"
    assert GPSConfig("relu", "gine", 32, 2, 4, 0.1, "layer", "node").task_level == "node"


MPNN_DEFAULT_NAMES = ["conv_layers.0.bias", "conv_layers.0.lin.weight", "conv_layers.1.bias", "conv_layers.1.lin.weight",
                      "conv_layers.2.bias", "conv_layers.2.lin.weight"]
_GPS_LAYER = ["conv.nn.0.weight", "conv.nn.0.bias", "conv.nn.2.weight", "conv.nn.2.bias", "conv.lin.weight",
              "conv.lin.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
              "norm1_local.weight", "norm1_local.bias", "norm1_attn.weight", "norm1_attn.bias", "ff_linear1.weight",
              "ff_linear1.bias", "ff_linear2.weight", "ff_linear2.bias", "norm2.weight", "norm2.bias"]
GPS_DEFAULT_NAMES = (["node_encoder.weight", "node_encoder.bias"] + [f"layers.{i}.{n}" for i in range(3) for n in _GPS_LAYER]
                     + ["lin_1.weight", "lin_1.bias", "lin_2.weight", "lin_2.bias"])


def test_default_configs_build_the_models_they_always_built():
    """The two name lists are the parent commit's ``named_parameters()`` of the default configs."""
    m = build_mpnn(MPNNConfig("gcn", "relu"), 9, 10)
    assert [n for n, _ in m.named_parameters()] == MPNN_DEFAULT_NAMES
    assert m.conv_layers[0].lin.weight.shape == (16, 9)
    assert not getattr(m, "layered_only", False) and m.encoder_kinds == (None, None)
    g = build_gps(GPSConfig("relu"), 9, 10)
    assert [n for n, _ in g.named_parameters()] == GPS_DEFAULT_NAMES
    assert g.node_encoder.weight.shape == (16, 9) and g.encoder_kinds == (None, None)
    # the same seed draws the same weights whether or not the new arguments are spelled out
    torch.manual_seed(4)
    a = build_mpnn(MPNNConfig("gcn", "relu"), 9, 10)
    torch.manual_seed(4)
    b = build_mpnn(MPNNConfig("gcn", "relu", node_encoder=None, edge_encoder=None), 9, 10)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_encoder_models_are_built_as_specified_and_are_layered_only():
    m = build_mpnn(MPNNConfig("gcn", "relu", hidden_channels=32, node_encoder="atom"), 9, 10)
    assert isinstance(m.node_encoder, AtomEncoder) and m.node_encoder.weight.shape == (174, 32)
    assert m.conv_layers[0].lin.weight.shape == (32, 32)                 # conv(H, H)
    assert m.layered_only is True and "node_encoder='atom'" in m.resident_reason()
    with pytest.raises(RuntimeError, match="categorical input encoder"):
        batching.refuse_layered_only(m, "the resident training step")
    e = build_mpnn(MPNNConfig("gine", "relu", node_encoder="atom", edge_encoder="bond"), 9, 10)
    assert isinstance(e.edge_encoder, BondEncoder) and e.edge_encoder.emb_dim == 16
    assert "edge_encoder='bond'" in e.resident_reason()
    g = build_gps(GPSConfig("relu", local_conv_type="gatedgcn", node_encoder="atom", edge_encoder="bond"), 9, 10)
    assert isinstance(g.node_encoder, AtomEncoder) and isinstance(g.edge_encoder, BondEncoder)
    assert g.layered_only and "categorical input encoder" in g.resident_reason() and "global attention" in g.resident_reason()
    g2 = build_gps(GPSConfig("relu", local_conv_type="gine", edge_encoder="bond"), 9, 10)
    assert isinstance(g2.edge_encoder, BondEncoder) and not isinstance(g2.node_encoder, AtomEncoder)


def test_to_device_keeps_integer_features_only_for_an_encoder_model():
    graphs = make_dataset("peptides_func", 2, seed=0, edge_features=True)
    assert graphs[0].x.dtype == torch.int64 and graphs[0].edge_attr.dtype == torch.int64

    def moved(model):
        return batching.to_device(model, Batch.from_data_list(graphs), "cpu")
    plain = moved(build_mpnn(MPNNConfig("gine", "relu"), 9, 10))
    assert plain.x.dtype == torch.float32 and plain.edge_attr.dtype == torch.float32
    atom = moved(build_mpnn(MPNNConfig("gine", "relu", node_encoder="atom"), 9, 10))
    assert atom.x.dtype == torch.int64 and atom.edge_attr.dtype == torch.float32
    both = moved(build_gps(GPSConfig("relu", "gatedgcn", node_encoder="atom", edge_encoder="bond"), 9, 10))
    assert both.x.dtype == torch.int64 and both.edge_attr.dtype == torch.int64
    assert torch.equal(both.x, Batch.from_data_list(graphs).x)
    bond = moved(build_gps(GPSConfig("relu", "gine", edge_encoder="bond"), 9, 10))
    assert bond.x.dtype == torch.float32 and bond.edge_attr.dtype == torch.int64
    b = Batch.from_data_list(graphs)
    b.x = b.x.float()
    with pytest.raises(TypeError, match="integer categories"):
        batching.to_device(build_mpnn(MPNNConfig("gcn", "relu", node_encoder="atom"), 9, 10), b, "cpu")


def test_header_and_binding_agree_on_the_new_names():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hscn.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(hscn_[a-z0-9_]+)\s*\(", src)) if n.startswith("hscn_catenc_"))
    assert declared == CATENC_NAMES
    assert sorted(n for n in _hip.exported_symbols() if n.startswith("hscn_catenc_")) == CATENC_NAMES
    lib = _hip.lib()
    for name in CATENC_NAMES:                            # one argument type per declared parameter
        params = re.search(r"\b%s\s*\(([^;{}]*)\)\s*;" % name, src).group(1).strip()
        count = 0 if params == "void" else len(params.split(","))
        assert len(_hip._SIGNATURES[name][1]) == count, name
        assert hasattr(lib, name)
    L, C = lib.hscn_catenc_long_row(), lib.hscn_catenc_chunk()
    assert 1 <= C <= L and lib.hscn_catenc_sort_chunk() % 64 == 0
    # argument checks come before any launch (no device needed)
    assert lib.hscn_catenc_fwd(None, None, None, None, -1, 3, 16, None, None) == -1
    assert lib.hscn_catenc_bwd(None, None, None, None, 4, 3, 13, 18, None, None, 0, None) == -3      # D % 4
    assert lib.hscn_catenc_bwd(None, None, None, None, 4, 3, 13, 16, None, None, 0, None) == -1      # NULL pointers
    assert lib.hscn_catenc_bwd_workspace_bytes(100, 3, 13, 16) == (-(-300 // C) + 13) * 16 * 4
