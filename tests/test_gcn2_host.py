"""GCNII without a device: GCN2Conv's beta, parameters and refusals, GCNIIConfig / build_gcnii, the surface the training
entry points read, the ABI declarations, the LDS plan against the library's, and the restatement of tests/gcn2_oracle.py
against a three-node example worked by hand."""
import ctypes
import math
import os
import re

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, GCNIIConfig, LapPEConfig, RWSEConfig, TrainingConfig
from graph_hscn.model.gcnii import GCNII, RESIDENT_REASON, build_gcnii
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GCN2Conv
from tests import gcn2_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hscn_gcn2_supported", "hscn_gcn2_plan", "hscn_gcn2_fwd", "hscn_gcn2_bwd", "hscn_gcn2_bwd_w_workspace_bytes",
           "hscn_gcn2_bwd_w")


def test_beta_is_log_theta_over_layer_plus_one_or_one():
    assert GCN2Conv(8, 0.1).beta == 1.0
    assert GCN2Conv(8, 0.1, theta=0.5).beta == 1.0 and GCN2Conv(8, 0.1, layer=3).beta == 1.0
    for theta, layer in ((0.5, 1), (0.5, 64), (1.0, 2), (1.5, 7)):
        c = GCN2Conv(8, 0.25, theta, layer)
        assert c.beta == math.log(theta / layer + 1.0) == GO.beta_of(theta, layer) and c.alpha == 0.25
    with pytest.raises(ValueError, match="beta must be in"):
        GCN2Conv(8, 0.1, theta=2.0, layer=1)                   # log 3 > 1


def test_state_dict_keys_are_pygs_and_the_weights_are_glorot():
    torch.manual_seed(0)
    shared, two = GCN2Conv(300, 0.1, 0.5, 2), GCN2Conv(300, 0.1, 0.5, 2, shared_weights=False)
    assert list(shared.state_dict()) == ["weight1"] and shared.weight2 is None
    assert list(two.state_dict()) == ["weight1", "weight2"]
    assert [n for n, _ in shared.named_parameters()] == ["weight1"]
    bound = math.sqrt(6.0 / 600.0)
    for w in (shared.weight1.detach(), two.weight1.detach(), two.weight2.detach()):
        assert tuple(w.shape) == (300, 300)
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.95 * bound
        assert abs(float(w.mean())) < 0.02 * bound and abs(float(w.std()) - bound / math.sqrt(3.0)) < 0.02 * bound
    assert not torch.equal(two.weight1, two.weight2)
    ref = GO.GCN2ConvRef(300, 0.1, 0.5, 2, shared_weights=False)
    two.load_state_dict(ref.state_dict(), strict=True)
    ref.load_state_dict(two.state_dict(), strict=True)


@pytest.mark.parametrize("kwargs,text", [(dict(cached=True), "cached=True"), (dict(normalize=False), "normalize=False"),
                                         (dict(add_self_loops=False), "add_self_loops=False")])
def test_constructor_refusals_are_by_name(kwargs, text):
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        GCN2Conv(16, 0.1, **kwargs)


def test_forward_refusals_are_by_name_before_any_launch():
    conv = GCN2Conv(8, 0.1)
    x, ei = torch.zeros(3, 8), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(NotImplementedError, match=re.escape("edge_weight=")):
        conv(x, x, ei, edge_weight=torch.ones(2))
    with pytest.raises(ValueError, match="act must be one of"):
        conv(x, x, ei, act="tanh")
    with pytest.raises(ValueError, match=r"x must be \[N, 8\]"):
        conv(torch.zeros(3, 12), x, ei)
    with pytest.raises(ValueError, match="x_0 must be"):
        conv(x, torch.zeros(2, 8), ei)


@pytest.mark.parametrize("H", [0, 2, 6, 301, 516, 1024])
def test_a_width_outside_the_envelope_is_refused_by_name(H):
    assert not Fh.gcn2_supported(H)
    with pytest.raises(ValueError, match="outside the kernel's envelope"):
        GCN2Conv(H, 0.1)
    with pytest.raises(ValueError, match="outside the GCN2Conv kernel's envelope"):
        GCNIIConfig("relu", hidden_channels=H)


def test_alpha_is_held_to_the_unit_interval():
    for a in (-0.1, 1.5, float("nan"), True, "0.1"):
        with pytest.raises(ValueError, match="alpha"):
            GCN2Conv(8, a)
    assert GCN2Conv(8, 0).alpha == 0.0 and GCN2Conv(8, 1).alpha == 1.0


def test_config_validation():
    cfg = GCNIIConfig("relu")
    assert (cfg.alpha, cfg.theta, cfg.shared_weights, cfg.residual, cfg.task_level) == (0.1, 0.5, True, False, "graph")
    assert cfg.node_encoder is None and cfg.pos_enc is None and cfg.pe_undirected is True
    assert not hasattr(cfg, "edge_encoder")
    assert GCNIIConfig("relu", hidden_channels=300).hidden_channels == 300
    assert GCNIIConfig("relu", theta=None).theta is None and GCNIIConfig("relu", alpha=0).alpha == 0
    bad = [dict(alpha=-0.1), dict(alpha=1.01), dict(alpha=True), dict(theta=0.0), dict(theta=-1.0), dict(theta=True),
           dict(theta=float("inf")), dict(num_layers=0), dict(num_layers=2.0), dict(hidden_channels=18),
           dict(hidden_channels=516), dict(task_level="edge"), dict(node_encoder="bond"), dict(activation="gelu"),
           dict(dropout=1.0), dict(shared_weights=1), dict(residual="yes"),
           dict(pos_enc=RWSEConfig(dim_in=9, dim_emb=32, dim_pe=4)), dict(pos_enc="rwse")]
    for args in bad:
        with pytest.raises(ValueError):
            GCNIIConfig(**{"activation": "relu", **args})
    pe = LapPEConfig(dim_in=9, dim_emb=16, dim_pe=4)
    assert GCNIIConfig("relu", pos_enc=pe).pos_enc is pe
    assert "gcnii" in open(os.path.join(ROOT, "graph-hscn_amd", "graph_hscn", "config", "config.py")).read().split(
        "class TrainingConfig")[1].split("model_type: str")[0]
    assert TrainingConfig("gcnii", "cross_entropy", "ap").model_type == "gcnii"


def test_build_gcnii_passes_every_field_through():
    pe = RWSEConfig(dim_in=9, dim_emb=20, dim_pe=4, ksteps=6)
    cfg = GCNIIConfig("tanh", hidden_channels=20, num_layers=5, dropout=0.3, alpha=0.2, theta=1.0, shared_weights=False,
                      residual=True, task_level="node", node_encoder="atom", pos_enc=pe, pe_undirected=False)
    m = build_gcnii(cfg, 9, 7)
    assert isinstance(m, GCNII) and m.num_layers == 5 == len(m.layers) and m.dropout == 0.3 and m.residual
    assert m.task_level == "node" and m.encoder_kinds == ("atom", None) and m.pos_enc is pe and not m.pe_undirected
    assert m.activation is ACT_DICT["tanh"] and m.head_width() == 7
    for l, conv in enumerate(m.layers, start=1):
        assert conv.layer == l and conv.alpha == 0.2 and conv.beta == math.log(1.0 / l + 1.0)
        assert conv.weight2 is not None and conv.channels == 20
    assert m.node_encoder.weight.shape[1] == 16                       # H - dim_pe beside the positional encoder
    keys = list(m.state_dict())
    assert "layers.0.weight1" in keys and "layers.4.weight2" in keys and "lin_1.weight" in keys and "lin_2.bias" in keys
    assert not any("edge_encoder" in k or "bias" in k for k in keys if k.startswith("layers."))
    plain = build_gcnii(GCNIIConfig("relu", hidden_channels=8, num_layers=2), 5, 3)
    assert list(plain.state_dict()) == ["node_encoder.weight", "node_encoder.bias", "layers.0.weight1",
                                        "layers.1.weight1", "lin_1.weight", "lin_1.bias", "lin_2.weight", "lin_2.bias"]
    twin = GO.GCNIIRef(5, 8, 3, 2)
    plain.load_state_dict(twin.state_dict(), strict=True)
    assert [c.beta for c in plain.layers] == [c.beta for c in twin.layers]


def test_the_resident_entry_points_are_told_why_not():
    from graph_hscn.train import batching
    m = GCNII(9, 16, 10, 3)
    assert m.layered_only is True and m.supported() is False and m.engine == "layered"
    assert m.resident_reason() == RESIDENT_REASON and "GCN2Conv" in RESIDENT_REASON
    with pytest.raises(RuntimeError, match=re.escape(m.resident_reason())):
        batching.refuse_layered_only(m, "the resident training step")
    with pytest.raises(RuntimeError, match=re.escape(RESIDENT_REASON)):
        batching.resident_step(m, None, "cross_entropy")
    pe = GCNII(9, 16, 10, 1, node_encoder="atom", pos_enc=RWSEConfig(dim_in=9, dim_emb=16, dim_pe=4))
    reason = pe.resident_reason()
    assert reason.startswith(RESIDENT_REASON) and "positional encoder" in reason and "node_encoder='atom'" in reason
    with pytest.raises(ValueError, match="at least one layer"):
        GCNII(9, 16, 10, 0)
    with pytest.raises(ValueError, match="task_level"):
        GCNII(9, 16, 10, 1, task_level="edge")


def test_every_task_level_takes_the_lrgb_width():
    from graph_hscn.model.gcnii import POOL_MAX_WIDTH
    assert POOL_MAX_WIDTH == 256 and POOL_MAX_WIDTH % 4 == 0           # slices of the mean pool stay multiples of 4
    for level in ("graph", "node", "link"):
        m = build_gcnii(GCNIIConfig("relu", hidden_channels=300, num_layers=1, task_level=level), 9, 12)
        assert m.head_width() == 12 and m.layers[0].channels == 300


def test_abi_is_still_24_and_the_new_symbols_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "hscn.h")).read()
    assert int(re.search(r"#define HSCN_ABI_VERSION (\d+)", src).group(1)) == 24 == _hip.ABI_VERSION
    assert "GCN2Conv (csrc/gcn2.hip).  Purely additive to ABI 24" in src
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _hip.lib()
    assert lib.hscn_abi_version() == 24
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, body), name
        assert name in _hip._SIGNATURES and hasattr(lib, name), name


def test_gcn2conv_is_exported_from_the_nn_package():
    import graph_hscn.nn as nn_pkg
    assert nn_pkg.GCN2Conv is GCN2Conv and "GCN2Conv" in nn_pkg.__all__


def test_the_plan_restated_in_python_is_the_librarys():
    lib = _hip.lib()
    for H in range(-4, 532):
        assert bool(lib.hscn_gcn2_supported(H)) == Fh.gcn2_supported(H), H
    buf = (ctypes.c_int32 * 4)()
    for shared in (True, False):
        for H in range(4, 516, 4):
            assert lib.hscn_gcn2_plan(H, 0 if shared else 1, buf) == 0
            p = Fh.gcn2_plan(H, shared)
            assert [int(v) for v in buf] == [p["row_tile"], p["panel"], int(p["resident"]), p["lds"]], (H, shared)
            assert p["lds"] <= Fh.GCN2_LDS_BYTES and p["panel"] % 16 == 0
            assert p["row_tile"] == (Fh.GCN2_ROW_TILE if shared else Fh.GCN2_ROW_TILE_TWO)
        assert lib.hscn_gcn2_plan(6, 0 if shared else 1, buf) == -3
    assert Fh.gcn2_resident_max_width(True) == 128 and Fh.gcn2_resident_max_width(False) == 96
    assert Fh.gcn2_plan(300)["panel"] == 32 and not Fh.gcn2_plan(300)["resident"]           # the LRGB width: two
    assert Fh.gcn2_plan(300)["lds"] <= Fh.GCN2_TWO_WG_BYTES                                 # workgroups a CU


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _hip.lib()
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 0, 16, 0.1, 1.0, 0, None) == 0
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 5, 16, 0.1, 1.0, 0, None) == -1
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 5, 18, 0.1, 1.0, 0, None) == -3
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 5, 16, 0.1, 1.0, 3, None) == -3
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 5, 16, 1.1, 1.0, 0, None) == -1
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, 5, 16, 0.1, 0.0, 0, None) == -1
    assert lib.hscn_gcn2_fwd(None, None, None, None, None, None, None, None, None, -1, 16, 0.1, 1.0, 0, None) == -1
    assert lib.hscn_gcn2_bwd(None, None, None, None, None, None, None, 0, 16, 0.1, 1.0, 0, None) == 0
    assert lib.hscn_gcn2_bwd(None, None, None, None, None, None, None, 5, 16, 0.1, 1.0, 0, None) == 0   # nothing asked
    assert lib.hscn_gcn2_bwd(None, None, None, None, ctypes.c_void_p(16), None, None, 5, 16, 0.1, 1.0, 0, None) == -1
    assert lib.hscn_gcn2_bwd(None, None, None, None, None, None, None, 5, 520, 0.1, 1.0, 0, None) == -3
    assert lib.hscn_gcn2_bwd_w(None, None, None, None, None, 5, 16, 0.1, None, 0, None) == -1
    assert lib.hscn_gcn2_bwd_w_workspace_bytes(100, 16) == lib.hscn_linear_bwd_w_workspace_bytes(100, 16, 16)


def test_the_restatement_against_a_three_node_example_by_hand():
    # edges 0 -> 1, 2 -> 1, 1 -> 0, and a listed self loop 2 -> 2 (dropped, then one loop per node): in-degrees with
    # loops: node 0: {1, 0} = 2, node 1: {0, 2, 1} = 3, node 2: {2} = 1
    ei = torch.tensor([[0, 2, 1, 2], [1, 1, 0, 2]])
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.5, 4.0]], dtype=torch.float64)
    x0 = torch.tensor([[0.0, 1.0], [2.0, 2.0], [-1.0, 0.5], [9.0, 9.0]], dtype=torch.float64)     # longer than x
    W1 = torch.tensor([[1.0, -2.0], [0.0, -1.0]], dtype=torch.float64)
    W2 = torch.tensor([[0.5, 0.0], [1.0, 1.0]], dtype=torch.float64)
    d = [2 ** -0.5, 3 ** -0.5, 1.0]
    p = torch.stack([d[0] * d[1] * x[1] + d[0] * d[0] * x[0],
                     d[1] * d[0] * x[0] + d[1] * d[2] * x[2] + d[1] * d[1] * x[1],
                     d[2] * d[2] * x[2]])
    assert torch.allclose(GO.propagate(x, ei), p, rtol=0, atol=1e-15)
    a, b = 0.25, math.log(0.5 / 2 + 1.0)
    h = 0.75 * p + 0.25 * x0[:3]
    hw = torch.stack([torch.stack([h[i, 0] * W1[0, 0] + h[i, 1] * W1[1, 0], h[i, 0] * W1[0, 1] + h[i, 1] * W1[1, 1]])
                      for i in range(3)])
    y = (1 - b) * h + b * hw
    assert torch.allclose(GO.gcn2(x, x0, ei, W1, None, a, b), y, rtol=0, atol=1e-14)
    assert torch.equal(GO.gcn2(x, x0, ei, W1, None, a, b, "relu"), torch.relu(GO.gcn2(x, x0, ei, W1, None, a, b)))
    assert bool((y < 0).any()) and bool((y > 0).any())
    two = (1 - b) * h + b * ((0.75 * p) @ W1 + (0.25 * x0[:3]) @ W2)
    assert torch.allclose(GO.gcn2(x, x0, ei, W1, W2, a, b), two, rtol=0, atol=1e-14)
    # the teeth's variant: edge 1 (2 -> 1) leaves the sum, the degrees stay
    p_skip = p.clone()
    p_skip[1] -= d[1] * d[2] * x[2]
    assert torch.allclose(GO.propagate(x, ei, skip_edge=1), p_skip, rtol=0, atol=1e-15)
    with pytest.raises(AssertionError):
        GO.propagate(x, ei, skip_edge=3)                          # a self loop is not a term of its own
    # alpha = 1: x does not enter; beta = 1 with alpha = 0: A_hat x W1
    assert torch.equal(GO.gcn2(x, x0, ei, W1, None, 1.0, b), GO.gcn2(x * 3 + 1, x0, ei, W1, None, 1.0, b))
    assert torch.allclose(GO.gcn2(x, x0, ei, W1, None, 0.0, 1.0), p @ W1, rtol=0, atol=1e-14)
