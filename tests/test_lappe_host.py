"""The LapPE encoder and the models' ``pos_enc`` without a device: config validation, parameter names and shapes, that a
model built without ``pos_enc`` is the model it was (tests/golden/posenc_parent_models.json: keys, shapes and SHA-256
of the initial values of every model below, recorded from the commit before ``pos_enc`` existed under the same
``torch.manual_seed``), the sign rule, the kernel's envelope, and the a-priori bound of tests/test_gpu_lappe.py held
against a float32 torch evaluation -- with its teeth."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, CONV_DICT
from tests import lappe_oracle as LO
from tests.helpers import f64_close

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posenc_parent_models.json")


def _lappe(**kw):
    from graph_hscn.config.config import LapPEConfig
    return LapPEConfig(**{**dict(dim_in=9, dim_emb=32, dim_pe=8), **kw})


# ---- config -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,needle", [
    (dict(model="Transformer"), "Transformer"),
    (dict(model="mlp"), "model must be 'DeepSet'"),
    (dict(raw_norm="batchnorm"), "raw_norm='batchnorm'"),
    (dict(raw_norm="layer"), "raw_norm must be 'none'"),
    (dict(eigen_max_freqs=0), "eigen_max_freqs=0"),
    (dict(eigen_max_freqs=65), "eigen_max_freqs=65"),
    (dict(dim_pe=6), "dim_pe=6"),
    (dict(dim_pe=0), "dim_pe=0"),
    (dict(dim_pe=36, dim_emb=64), "dim_pe=36"),
    (dict(layers=0), "layers=0"),
    (dict(layers=5), "layers=5"),
    (dict(post_layers=-1), "post_layers"),
    (dict(dim_pe=32, dim_emb=32), "too large"),
])
def test_config_refusals_name_what_they_refuse(kw, needle):
    with pytest.raises(ValueError, match=needle):
        _lappe(**kw)


def test_config_defaults_are_the_published_ones():
    c = _lappe()
    assert (c.model, c.layers, c.post_layers, c.eigen_max_freqs, c.eigvec_norm, c.eigen_laplacian_norm, c.raw_norm,
            c.sign_flip, c.pass_as_var) == ("DeepSet", 2, 0, 10, "L2", "none", "none", True, False)


# ---- parameters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,post,expand", [(1, 0, True), (2, 0, True), (3, 1, False), (4, 2, True)])
def test_encoder_state_dict(layers, post, expand):
    from graph_hscn.encoder import LapPENodeEncoder
    enc = LapPENodeEncoder(_lappe(layers=layers, post_layers=post), 9, 32, expand_x=expand)
    w = LO.widths(8, layers)
    want = {"linear_A.weight": (w[1], 2), "linear_A.bias": (w[1],)}
    for i, (a, b) in enumerate(zip(w[1:-1], w[2:])):
        want[f"pe_encoder.{i}.weight"], want[f"pe_encoder.{i}.bias"] = (b, a), (b,)
    pw = [8] + [16] * (post - 1) + [8] if post else [8]
    for i, (a, b) in enumerate(zip(pw[:-1], pw[1:])):
        want[f"post_mlp.{i}.weight"], want[f"post_mlp.{i}.bias"] = (b, a), (b,)
    if expand:
        want["linear_x.weight"], want["linear_x.bias"] = (24, 9), (24,)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want


def _models():
    """name -> constructor of every model whose parameters the parent commit fixed (no ``pos_enc``)."""
    from graph_hscn.model.gps import GPS
    from graph_hscn.model.mpnn import MPNN
    relu = ACT_DICT["relu"]
    return {
        "gps_plain": lambda **kw: GPS(9, 32, 10, 2, 4, None, relu, **kw),
        "gps_gine": lambda **kw: GPS(9, 32, 10, 2, 4, "gine", relu, **kw),
        "gps_atom": lambda **kw: GPS(9, 32, 10, 2, 4, None, relu, node_encoder="atom", **kw),
        "gps_atom_bond_gatedgcn": lambda **kw: GPS(9, 32, 10, 2, 4, "gatedgcn", relu, node_encoder="atom",
                                                   edge_encoder="bond", **kw),
        "gps_spd": lambda **kw: GPS(9, 32, 10, 2, 4, "gcn", relu, attn_bias="spd", **kw),
        "gps_exphormer": lambda **kw: GPS(9, 32, 10, 2, 4, "gine", relu, global_model="exphormer", **kw),
        "mpnn_gcn": lambda **kw: MPNN(CONV_DICT["gcn"], relu, 9, 32, 10, 3, **kw),
        "mpnn_atom_gatedgcn": lambda **kw: MPNN(CONV_DICT["gatedgcn"], relu, 9, 32, 10, 3, node_encoder="atom",
                                                edge_encoder="bond", **kw),
        "mpnn_gat_ln": lambda **kw: MPNN(CONV_DICT["gat"], relu, 9, 32, 10, 3, use_layer_norm=True, **kw),
        "mpnn_transformerconv": lambda **kw: MPNN(CONV_DICT["transformerconv"], relu, 9, 32, 10, 3, heads=4, **kw),
    }


def _fingerprint(model):
    lazy = torch.nn.parameter.UninitializedParameter
    # a Linear(-1, D) draws nothing until its first use: its bias is memory as allocated, only the shape is compared
    unset = tuple(n + "." for n, mod in model.named_modules() if isinstance(getattr(mod, "weight", None), lazy))
    out = []
    for k, v in model.state_dict().items():
        if isinstance(v, lazy):
            out.append([k, None, None])
        elif k.startswith(unset):
            out.append([k, list(v.shape), None])
        else:
            out.append([k, list(v.shape), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()])
    return out


def record_parent_fingerprints():
    """What wrote the golden file, run on the commit before ``pos_enc`` existed."""
    res = {}
    for name, make in _models().items():
        torch.manual_seed(1234)
        res[name] = _fingerprint(make())
    return res


@pytest.mark.parametrize("name", ["gps_plain", "gps_gine", "gps_atom", "gps_atom_bond_gatedgcn", "gps_spd",
                                  "gps_exphormer", "mpnn_gcn", "mpnn_atom_gatedgcn", "mpnn_gat_ln",
                                  "mpnn_transformerconv"])
def test_a_model_without_pos_enc_is_the_model_it_was(name):
    want = json.load(open(GOLDEN))[name]
    torch.manual_seed(1234)
    m = _models()[name]()
    assert _fingerprint(m) == want
    assert m.pos_enc is None and not hasattr(m, "pe_encoder") and not hasattr(m, "linear_x")
    assert "positional encoder" not in (m.resident_reason() or "")
    torch.manual_seed(1234)                        # the same through pos_enc=None spelled out
    assert _fingerprint(_models()[name](pos_enc=None, pe_undirected=True)) == want


@pytest.mark.parametrize("kind", ["lappe", "rwse"])
@pytest.mark.parametrize("name", ["gps_atom", "gps_atom_bond_gatedgcn", "gps_gine", "gps_spd", "gps_exphormer",
                                  "mpnn_gcn", "mpnn_atom_gatedgcn"])
def test_models_with_pos_enc_own_the_encoder_behind_their_parameters(name, kind):
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.model import _common
    cfg = _lappe(post_layers=1) if kind == "lappe" else RWSEConfig(dim_in=9, dim_emb=32, dim_pe=8, model="mlp", layers=2)
    base = _models()[name]()
    m = _models()[name](pos_enc=cfg)
    keys, base_keys = list(m.state_dict()), list(base.state_dict())
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()
              if not isinstance(v, torch.nn.parameter.UninitializedParameter)}
    own = [k for k in keys if k.startswith(("pe_encoder.", "linear_x."))]
    assert keys[:len(base_keys)] == base_keys and keys[len(base_keys):] == own      # created after everything else
    if name.startswith("mpnn") and "atom" not in name:
        assert shapes["linear_x.weight"] == (24, 9) and shapes["conv_layers.0.lin.weight"][1] == 32
    else:
        assert "linear_x.weight" not in shapes
    if "atom" in name:                             # the AtomEncoder table has D - dim_pe columns
        assert shapes["node_encoder.weight"][1] == 24
    elif name.startswith("gps"):
        assert shapes["node_encoder.weight"] == (24, 9)
    if kind == "lappe":
        assert shapes["pe_encoder.linear_A.weight"] == (16, 2) and shapes["pe_encoder.pe_encoder.0.weight"] == (8, 16)
        assert shapes["pe_encoder.post_mlp.0.weight"] == (8, 8)
    else:
        assert shapes["pe_encoder.pe_encoder.0.weight"] == (16, 20) and shapes["pe_encoder.pe_encoder.1.weight"] == (8, 16)
    assert m.layered_only is True
    assert "positional encoder" in m.resident_reason()
    assert _common.POSENC_RESIDENT_REASON in m.resident_reason()
    assert callable(m.encode_nodes)


def test_dim_emb_must_be_the_hidden_width():
    from graph_hscn.config.config import GPSConfig, MPNNConfig
    from graph_hscn.model.gps import build_gps
    from graph_hscn.model.mpnn import build_mpnn
    cfg = _lappe(dim_emb=64)
    for make in (_models()["gps_atom"], _models()["mpnn_gcn"]):
        with pytest.raises(ValueError, match=r"64.*32"):
            make(pos_enc=cfg)
    with pytest.raises(ValueError, match=r"64.*32"):
        GPSConfig("relu", None, 32, pos_enc=cfg)
    with pytest.raises(ValueError, match=r"64.*32"):
        MPNNConfig("gcn", "relu", 32, pos_enc=cfg)
    with pytest.raises(ValueError, match="LapPEConfig"):
        _models()["gps_atom"](pos_enc=object())
    ok = _lappe(dim_in=123)                        # dim_in is not read
    g = build_gps(GPSConfig("relu", "gatedgcn", 32, 2, 4, node_encoder="atom", edge_encoder="bond", pos_enc=ok), 9, 10)
    m = build_mpnn(MPNNConfig("gcn", "relu", 32, 3, pos_enc=ok, pe_undirected=False), 9, 10)
    assert g.pos_enc is ok and m.pos_enc is ok and m.pe_undirected is False and g.pe_undirected is True


def test_a_vec_that_requires_grad_is_refused_by_name():
    from graph_hscn.nn import functional as Fh
    vec, val, Ws, bs, _ = LO.make_inputs(3, 4, 4, 1, 0)
    with pytest.raises(ValueError, match="vec requires grad"):
        Fh.LapPEDeepSetFn.apply(vec.requires_grad_(True), val, Ws, bs, None)
    with pytest.raises(ValueError, match="val requires grad"):
        Fh.LapPEDeepSetFn.apply(vec.detach(), val.requires_grad_(True), Ws, bs, None)


# ---- the sign rule ----------------------------------------------------------------------------------------------------
def test_sign_rule_against_the_published_philox_vectors():
    from tests.test_gpu_exact_edges import philox4x32_10
    # Random123's known answer for counter 0 under key 0 has word 0 = 0x6627e8d5 < 2^31: frequency 0 keeps its sign
    assert int(philox4x32_10(np.zeros((1, 4), dtype=np.uint64), (0, 0))[0, 0]) == 0x6627E8D5
    assert float(LO.signs(1, 0)[0]) == 1.0
    assert torch.equal(LO.signs(7, None), torch.ones(7, dtype=torch.float64))
    for seed in (0, 1, 0x1234567887654321, 2 ** 64 - 1):
        ctr = np.zeros((64, 4), dtype=np.uint64)
        ctr[:, 0] = np.arange(64)
        w0 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[:, 0]
        want = torch.tensor([-1.0 if int(w) >= 2 ** 31 else 1.0 for w in w0], dtype=torch.float64)
        got = LO.signs(64, seed)
        assert torch.equal(got, want)
        assert torch.equal(got[:10], LO.signs(10, seed))          # a column's sign does not depend on K
        assert 8 <= int((got < 0).sum()) <= 56                     # both signs occur


# ---- the envelope -----------------------------------------------------------------------------------------------------
def test_envelope_at_both_sides_of_every_edge():
    from graph_hscn.nn import functional as Fh
    lib = _hip.lib()
    for K, dp, L, want in [(1, 4, 1, 1), (64, 32, 4, 1), (10, 16, 2, 1), (0, 16, 2, 0), (65, 16, 2, 0), (10, 0, 2, 0),
                           (10, 4, 2, 1), (10, 3, 2, 0), (10, 5, 2, 0), (10, 28, 2, 1), (10, 32, 2, 1), (10, 36, 2, 0),
                           (10, 16, 0, 0), (10, 16, 1, 1), (10, 16, 4, 1), (10, 16, 5, 0), (-1, 16, 2, 0)]:
        assert lib.hscn_lappe_supported(K, dp, L) == want, (K, dp, L)
        assert Fh.lappe_supported(K, dp, L) == bool(want), (K, dp, L)
    assert lib.hscn_lappe_tile() == 64
    # one partial gradient per workgroup, one workgroup per 256 samples, at most 512 workgroups
    params = 3 * 32 + 33 * 16
    assert lib.hscn_lappe_workspace_floats(1, 10, 16, 2) == params
    assert lib.hscn_lappe_workspace_floats(64, 10, 16, 2) == 3 * params
    assert lib.hscn_lappe_workspace_floats(20000, 10, 16, 2) == 512 * params
    assert lib.hscn_lappe_workspace_floats(5, 10, 6, 2) == 0
    # argument checks come before any launch: no device is needed to be refused
    table = (_hip.ctypes.c_void_p * 4)()
    assert lib.hscn_lappe_fwd(None, None, table, -1, 10, 16, 2, 0, 0, None, None) == -1
    assert lib.hscn_lappe_fwd(None, None, table, 0, 10, 6, 2, 0, 0, None, None) == -3
    assert lib.hscn_lappe_fwd(None, None, table, 0, 10, 16, 2, 0, 0, None, None) == -1      # null parameters


# ---- the bound of the GPU test, held by a float32 evaluation ----------------------------------------------------------
SHAPES = [(1, 4, 1, 5), (2, 16, 10, 200), (3, 32, 64, 130), (4, 8, 4, 65)]


@pytest.mark.parametrize("layers,dim_pe,K,N", SHAPES)
def test_float32_holds_the_a_priori_bound_and_the_bound_has_teeth(layers, dim_pe, K, N):
    vec, val, Ws, bs, _ = LO.make_inputs(N, K, dim_pe, layers, seed=layers * 100 + K)
    sg = LO.signs(K, 77)
    ref, _, _ = LO.chain(vec, val, Ws, bs, sg)
    mag, _, _ = LO.chain(vec, val, Ws, bs, sg, absolute=True)
    got, _, _ = LO.chain(vec, val, Ws, bs, sg, dtype=torch.float32)
    n = LO.bound_n(dim_pe, layers, K)
    assert got.dtype == torch.float32
    assert f64_close(got, ref, mag, n, what="float32 restatement")
    assert float(ref[1].abs().max()) == 0.0 if N >= 3 else True            # the all-NaN row
    dropped, _, _ = LO.chain(vec, val, Ws, bs, sg, drop_freq=0)
    assert not f64_close(got, dropped, mag, n), "the bound cannot see a dropped frequency"
    rev = sg.clone()
    rev[0] = -rev[0]
    flipped, _, _ = LO.chain(vec, val, Ws, bs, rev)
    assert not f64_close(got, flipped, mag, n), "the bound cannot see a reversed sign"


@pytest.mark.parametrize("layers,dim_pe,K,N", SHAPES)
def test_hand_written_gradients_are_autograd_s(layers, dim_pe, K, N):
    vec, val, Ws, bs, g = LO.make_inputs(N, K, dim_pe, layers, seed=5)
    sg = LO.signs(K, 3)
    _, grads, _ = LO.chain(vec, val, Ws, bs, sg, g=g)
    leaves = [t.double().requires_grad_(True) for wb in zip(Ws, bs) for t in wb]
    u = torch.stack((torch.nan_to_num(vec.double()) * sg, torch.nan_to_num(val.double())), 2)
    a = u
    for W, b in zip(leaves[0::2], leaves[1::2]):
        a = torch.relu(a @ W.t() + b)
    ((a * (~torch.isnan(vec)).unsqueeze(2)).sum(1) * g.double()).sum().backward()
    for hand, leaf in zip(grads, leaves):
        assert float((hand - leaf.grad).abs().max()) <= 1e-12 * max(1.0, float(leaf.grad.abs().max()))
