"""The three layered-only models (GPS, SAN, GCNII) and their configs without a device, across the change that gave them
one base class (model/_common.py LayeredModel) and the configs shared checks: the parameters are the ones they were
(tests/golden/layered_models_parent.json: keys in order, shapes and SHA-256 of the initial values, recorded from the
commit before the base existed under the same ``torch.manual_seed``; tests/test_lappe_host.py holds the models that file
already covered), the surface ``train.batching`` and ``train.train`` use answers what it answered, and every config
refusal keeps its type and its text (the literals below were captured on that commit too)."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from graph_hscn.config.config import ACT_DICT, GCNIIConfig, GPSConfig, HSCNConfig, LapPEConfig, MPNNConfig, RWSEConfig, SANConfig
from graph_hscn.encoder.categorical import resident_reason as encoder_reason
from graph_hscn.model import _common, gcnii, gps, san
from graph_hscn.model.gcnii import GCNII
from graph_hscn.model.gps import GPS
from graph_hscn.model.san import SAN
from tests.test_lappe_host import _fingerprint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layered_models_parent.json")
RELU = ACT_DICT["relu"]


def _lappe(D=32):
    return LapPEConfig(dim_in=9, dim_emb=D, dim_pe=8, post_layers=1)


def _rwse(D=32):
    return RWSEConfig(dim_in=9, dim_emb=D, dim_pe=8, model="mlp", layers=2)


# ---- parameters, names, order and RNG draws ---------------------------------------------------------------------------
MODELS = {
    "san_default": lambda: SAN(9, 32, 10, 2, 4, RELU),
    "san_real_pairs_only": lambda: SAN(9, 32, 10, 2, 4, RELU, full_graph=False),
    "san_atom_bond": lambda: SAN(9, 32, 10, 2, 4, RELU, node_encoder="atom", edge_encoder="bond"),
    "san_rwse": lambda: SAN(9, 32, 10, 2, 4, RELU, pos_enc=_rwse()),
    "gcnii_default": lambda: GCNII(9, 32, 10, 3, RELU),
    "gcnii_two_weights": lambda: GCNII(9, 32, 10, 3, RELU, shared_weights=False),
    "gcnii_atom": lambda: GCNII(9, 32, 10, 3, RELU, node_encoder="atom"),
    "gcnii_lappe": lambda: GCNII(9, 32, 10, 3, RELU, pos_enc=_lappe()),
    "gcnii_300": lambda: GCNII(9, 300, 10, 2, RELU),
    "gps_dense_lappe": lambda: GPS(9, 32, 10, 2, 4, "gatedgcn", RELU, node_encoder="atom", edge_encoder="bond",
                                   pos_enc=_lappe()),
    "gps_exphormer_gine_rwse": lambda: GPS(9, 32, 10, 2, 4, "gine", RELU, global_model="exphormer", pos_enc=_rwse()),
}


def record_parent_fingerprints():
    """What wrote the golden file, run on the commit before ``LayeredModel`` existed."""
    res = {}
    for name, make in MODELS.items():
        torch.manual_seed(1234)
        res[name] = _fingerprint(make())
    return res


@pytest.mark.parametrize("name", list(MODELS))
def test_a_model_is_the_model_it_was(name):
    want = json.load(open(GOLDEN))[name]
    torch.manual_seed(1234)
    assert _fingerprint(MODELS[name]()) == want


def test_the_golden_file_covers_what_it_says():
    want = json.load(open(GOLDEN))
    assert set(want) == set(MODELS)
    keys = {name: [k for k, _, _ in rows] for name, rows in want.items()}
    assert "exph_edge_encoder.weight" in keys["gps_exphormer_gine_rwse"]
    assert keys["gps_exphormer_gine_rwse"][-1].startswith("pe_encoder.") and keys["san_rwse"][-1].startswith("pe_encoder.")
    assert "fake_edge_emb.weight" in keys["san_default"] and "fake_edge_emb.weight" not in keys["san_real_pairs_only"]
    first_layer_key = next(i for i, k in enumerate(keys["san_default"]) if k.startswith("layers."))
    assert keys["san_default"].index("edge_encoder.weight") < keys["san_default"].index("fake_edge_emb.weight") < first_layer_key
    assert "layers.0.weight2" in keys["gcnii_two_weights"] and "layers.0.weight2" not in keys["gcnii_default"]


# ---- the surface ------------------------------------------------------------------------------------------------------
# name -> (constructor taking keywords, the model's own constant, the head width asked for)
SURFACE = {
    "gps": (lambda **kw: GPS(9, 32, 10, 1, 4, "gine", RELU, **kw), gps.RESIDENT_REASON),
    "gps_exphormer": (lambda **kw: GPS(9, 32, 10, 1, 4, "gine", RELU, global_model="exphormer", **kw),
                      gps.EXPHORMER_RESIDENT_REASON),
    "san": (lambda **kw: SAN(9, 32, 10, 1, 4, RELU, **kw), san.RESIDENT_REASON),
    "gcnii": (lambda **kw: GCNII(9, 32, 10, 1, RELU, **kw), gcnii.RESIDENT_REASON),
}


def test_the_constants_say_what_they_said():
    assert gps.RESIDENT_REASON.startswith("global attention (model/gps.py GPS): per-graph multi-head self-attention has no")
    assert gps.EXPHORMER_RESIDENT_REASON.startswith("Exphormer's sparse attention (model/gps.py GPS, global_model='exphormer')")
    assert san.RESIDENT_REASON.startswith("SAN's attention over real and fake edges (model/san.py SAN): full-graph")
    assert gcnii.RESIDENT_REASON.startswith("GCNII's layers (model/gcnii.py GCNII): a GCN2Conv stack that reads the initial")
    for text in (gps.RESIDENT_REASON, gps.EXPHORMER_RESIDENT_REASON, san.RESIDENT_REASON, gcnii.RESIDENT_REASON):
        assert text.endswith("has no one-launch, resident or captured form; the model runs on the layered operators")


@pytest.mark.parametrize("name", list(SURFACE))
def test_resident_reason_supported_and_head_width(name):
    make, constant = SURFACE[name]
    plain, with_pe = make(), make(pos_enc=_rwse())
    both = make(pos_enc=_lappe(), node_encoder="atom")
    assert plain.resident_reason() == constant
    assert plain.resident_reason(object(), need_grad=True) == constant
    assert with_pe.resident_reason() == constant + "; " + _common.POSENC_RESIDENT_REASON
    assert both.resident_reason() == constant + "; " + _common.POSENC_RESIDENT_REASON + "; " + encoder_reason("atom", None)
    for m in (plain, with_pe, both):
        assert m.supported() is False and m.supported(object()) is False
        assert m.head_width() == 10 and m.layered_only is True
        assert m.engine == "layered" and m.last_engine is None and m.dropout_seed is None


@pytest.mark.parametrize("name", list(SURFACE))
def test_the_engine_is_checked_before_the_batch_is_read(name):
    make, constant = SURFACE[name]
    for m in (make(), make(pos_enc=_rwse(), node_encoder="atom")):
        m.engine = "resident"
        with pytest.raises(RuntimeError) as err:
            m(None)
        assert str(err.value) == f"engine='resident' does not take this model: {m.resident_reason()}"
        assert constant in str(err.value)
        m.engine = "bogus"
        with pytest.raises(ValueError) as err:
            m(None)
        assert str(err.value) == "engine must be 'layered', 'auto' or 'resident', got 'bogus'"
        assert m.last_engine is None


def test_one_pool_and_one_table_for_the_three():
    assert GPS._pool is SAN._pool is GCNII._pool is _common.LayeredModel._pool
    assert gcnii.POOL_MAX_WIDTH == 256 == _common.POOL_MAX_WIDTH
    assert gps._Table is _common._Table
    for cls in (GPS, SAN, GCNII):
        assert issubclass(cls, _common.LayeredModel)
        for name in ("resident_reason", "supported", "head_width", "check_flags", "_embed_x", "_head", "_forward", "_pool"):
            assert name not in vars(cls), (cls.__name__, name)


HINT = " and the batch carries no edge_attr (Data(edge_attr=[E, De]); make_dataset(..., edge_features=True))"


def test_a_missing_edge_attr_is_refused_in_the_model_s_own_words():
    with pytest.raises(ValueError) as err:
        GPS(9, 32, 10, 1, 4, "gine", RELU)._edge_attr(SimpleNamespace())
    assert str(err.value) == "the model has edge-aware convolutions (local_conv 'gine')" + HINT
    with pytest.raises(ValueError) as err:
        SAN(9, 32, 10, 1, 4, RELU)._edge_attr(SimpleNamespace(edge_attr=None))
    assert str(err.value) == "SAN's real pairs are scored through their edge features" + HINT
    ints = torch.zeros(3, 3, dtype=torch.long)
    assert SAN(9, 32, 10, 1, 4, RELU, edge_encoder="bond")._edge_attr(SimpleNamespace(edge_attr=ints)) is ints
    with pytest.raises(TypeError, match="edge_attr must be float32"):
        SAN(9, 32, 10, 1, 4, RELU)._edge_attr(SimpleNamespace(edge_attr=ints))


@pytest.mark.parametrize("cls", [GPS, SAN, GCNII])
def test_the_shared_refusals_of_the_models_keep_their_texts_and_their_order(cls):
    depth = f"{cls.__name__} needs at least one layer"
    with pytest.raises(ValueError) as err:
        cls(9, 32, 10, 0)
    assert str(err.value) == depth
    with pytest.raises(ValueError) as err:                     # the task level is looked at before the depth
        cls(9, 32, 10, 0, task_level="edge")
    assert str(err.value) == "task_level must be 'graph', 'node' or 'link', not 'edge'"
    with pytest.raises(ValueError) as err:                     # and the encoders before the task level
        cls(9, 32, 10, 0, task_level="edge", node_encoder="residue")
    assert str(err.value) == "node_encoder must be one of ['atom'] or None, not 'residue'"
    with pytest.raises(ValueError) as err:                     # the activation after the depth
        cls(9, 32, 10, 0, activation=torch.relu)
    assert str(err.value) == depth
    with pytest.raises(ValueError) as err:
        cls(9, 32, 10, 1, activation=torch.relu)
    assert str(err.value) == "activation must be one of config.ACT_DICT's (it runs in a Linear's epilogue)"


# ---- the configs' refusals, word for word ----------------------------------------------------------------------------
TASK = "task_level must be 'graph', 'node' or 'link', got 'edge'"
NODE_ENC = "node_encoder must be one of ('atom',) or None, got 'residue'"
EDGE_ENC = "edge_encoder must be one of ('bond',) or None, got 'residue'"
ACTIVATION = "activation must be one of ['elu', 'identity', 'relu', 'tanh'], got 'swish'"
NORM = "norm must be 'layer', 'batch' or None, got 'group'"
POSITIVE = "0 must be positive."
INDIVISIBLE = "hidden_channels 30 must be divisible by num_heads 4."
WIDTH = "head width {} (hidden_channels / num_heads) must be a multiple of 4 in [4, 64] and hidden_channels at most 512."
DEGREE = "expander_degree must be an even integer in [2, 32], got {}"
VIRTUAL = "num_virtual_nodes must be an integer in [0, 4], got {}"

CONFIG_REFUSALS = [
    (MPNNConfig, ("gcn", "relu"), {"task_level": "edge"}, TASK),
    (MPNNConfig, ("gcn", "relu"), {"node_encoder": "residue"}, NODE_ENC),
    (MPNNConfig, ("gcn", "relu"), {"edge_encoder": "residue"}, EDGE_ENC),
    (MPNNConfig, ("gcn", "relu"), {"edge_encoder": "bond"},
     "edge_encoder='bond' needs an edge-aware convolution ('gine', 'gatedgcn', 'transformerconv_edge', 'pna_edge'), got 'gcn'"),
    (MPNNConfig, ("gcn", "relu"), {"dropout": 1.5}, "1.5 must be between 0.0 and 1.0."),
    (HSCNConfig, ("relu",), {"task_level": "edge"}, TASK),
    (GPSConfig, ("relu",), {"task_level": "edge"}, TASK),
    (GPSConfig, ("relu",), {"node_encoder": "residue"}, NODE_ENC),
    (GPSConfig, ("relu",), {"edge_encoder": "residue"}, EDGE_ENC),
    (GPSConfig, ("relu", None), {"edge_encoder": "bond"},
     "edge_encoder='bond' needs an edge-aware convolution ('gine', 'gatedgcn', 'transformerconv_edge', 'pna_edge'), got None"),
    (GPSConfig, ("relu",), {"dropout": 1.0}, "1.0 must be in [0.0, 1.0)."),
    (GPSConfig, ("relu",), {"dropout": -0.5}, "-0.5 must be in [0.0, 1.0)."),
    (GPSConfig, ("relu",), {"num_layers": 0}, POSITIVE),
    (GPSConfig, ("relu",), {"num_heads": 0}, POSITIVE),
    (GPSConfig, ("relu",), {"hidden_channels": 0}, POSITIVE),
    (GPSConfig, ("relu",), {"norm": "group"}, NORM),
    (GPSConfig, ("relu",), {"hidden_channels": 30}, INDIVISIBLE),
    (GPSConfig, ("relu",), {"hidden_channels": 40}, WIDTH.format(10)),
    (GPSConfig, ("relu",), {"hidden_channels": 8, "num_heads": 4}, WIDTH.format(2)),
    (GPSConfig, ("relu",), {"hidden_channels": 576, "num_heads": 9}, WIDTH.format(64)),
    (GPSConfig, ("relu",), {"hidden_channels": 272, "num_heads": 4}, WIDTH.format(68)),
    (GPSConfig, ("relu",), {"expander_degree": 34}, DEGREE.format(34)),
    (GPSConfig, ("relu",), {"expander_degree": 3}, DEGREE.format(3)),
    (GPSConfig, ("relu",), {"expander_degree": 0}, DEGREE.format(0)),
    (GPSConfig, ("relu",), {"expander_degree": True}, DEGREE.format(True)),
    (GPSConfig, ("relu",), {"num_virtual_nodes": 5}, VIRTUAL.format(5)),
    (GPSConfig, ("relu",), {"num_virtual_nodes": -1}, VIRTUAL.format(-1)),
    # where two checks could both fire, the one that fired first still does
    (GPSConfig, ("relu",), {"expander_degree": 34, "num_virtual_nodes": 5}, DEGREE.format(34)),
    (GPSConfig, ("relu",), {"dropout": 1.0, "num_layers": 0, "norm": "group"}, "1.0 must be in [0.0, 1.0)."),
    (GPSConfig, ("relu",), {"num_layers": 0, "hidden_channels": 30}, POSITIVE),
    (SANConfig, ("relu",), {"task_level": "edge"}, TASK),
    (SANConfig, ("swish",), {}, ACTIVATION),
    (SANConfig, ("swish",), {"task_level": "edge"}, TASK),
    (SANConfig, ("swish",), {"node_encoder": "residue"}, ACTIVATION),
    (SANConfig, ("relu",), {"node_encoder": "residue"}, NODE_ENC),
    (SANConfig, ("relu",), {"edge_encoder": "residue"}, EDGE_ENC),
    (SANConfig, ("relu",), {"node_encoder": "residue", "edge_encoder": "residue"}, NODE_ENC),
    (SANConfig, ("relu",), {"dropout": 1.0}, "1.0 must be in [0.0, 1.0)."),
    (SANConfig, ("relu",), {"dropout": -0.5}, "-0.5 must be in [0.0, 1.0)."),
    (SANConfig, ("relu",), {"num_layers": 0}, POSITIVE),
    (SANConfig, ("relu",), {"num_heads": 0}, POSITIVE),
    (SANConfig, ("relu",), {"norm": "group"}, NORM),
    (SANConfig, ("relu",), {"hidden_channels": 30}, INDIVISIBLE),
    (SANConfig, ("relu",), {"hidden_channels": 40}, WIDTH.format(10)),
    (SANConfig, ("relu",), {"hidden_channels": 576, "num_heads": 9}, WIDTH.format(64)),
    (SANConfig, ("relu",), {"dropout": 1.0, "gamma": -1.0}, "gamma must be a finite number >= 0, got -1.0"),
    (SANConfig, ("relu",), {"norm": "group", "hidden_channels": 30}, NORM),
    (GCNIIConfig, ("relu",), {"task_level": "edge"}, TASK),
    (GCNIIConfig, ("swish",), {}, ACTIVATION),
    (GCNIIConfig, ("swish",), {"node_encoder": "residue"}, ACTIVATION),
    (GCNIIConfig, ("relu",), {"node_encoder": "residue"}, NODE_ENC),
    (GCNIIConfig, ("relu",), {"dropout": 1.5}, "1.5 must be in [0.0, 1.0)."),
    (GCNIIConfig, ("relu",), {"dropout": 1.0, "num_layers": 0}, "1.0 must be in [0.0, 1.0)."),
    (GCNIIConfig, ("relu",), {"num_layers": 0}, "num_layers must be an int >= 1, got 0"),
]


@pytest.mark.parametrize("cls,args,kw,text", CONFIG_REFUSALS,
                         ids=[f"{c.__name__}-{a[0]}-{'-'.join(k)}" for c, a, k, _ in CONFIG_REFUSALS])
def test_config_refusals_word_for_word(cls, args, kw, text):
    with pytest.raises(ValueError) as err:
        cls(*args, **kw)
    assert type(err.value) is ValueError and str(err.value) == text


def test_what_a_config_does_not_check_it_still_does_not_check():
    assert GPSConfig("not-an-activation").activation == "not-an-activation"
    assert GPSConfig("relu", dropout=0).dropout == 0 and SANConfig("relu", dropout=0.0).dropout == 0.0
    assert MPNNConfig("gcn", "relu", dropout=1.0).dropout == 1.0           # MPNN's own rule admits 1.0
    assert MPNNConfig("gcn", "relu", num_layers=0).num_layers == 0 and HSCNConfig("relu", num_layers=0).num_layers == 0
    assert SANConfig("ReLU").activation == "ReLU" and GCNIIConfig("Tanh").activation == "Tanh"


def test_the_exphormer_arguments_are_checked_by_one_function_with_the_kernels_bounds():
    from graph_hscn.nn import functional as Fh
    assert (Fh.EXPANDER_MAX_DEGREE, Fh.EXPH_MAX_VIRTUAL_NODES) == (32, 4)   # what the literal texts above spell out
    for kw in ({"expander_degree": 34}, {"expander_degree": 5}, {"num_virtual_nodes": 5}, {"num_virtual_nodes": True}):
        with pytest.raises(ValueError) as of_config:
            GPSConfig("relu", **kw)
        with pytest.raises(ValueError) as of_model:
            GPS(9, 32, 10, 1, global_model="exphormer", **kw)
        assert str(of_config.value) == str(of_model.value)
    GPS(9, 32, 10, 1, expander_degree=34)                                   # the dense model does not read it
