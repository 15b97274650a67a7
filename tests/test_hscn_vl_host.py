"""HSCN's opt-in ("virtual", "to", "local") relation: config / builder / state_dict surface, the envelope answers of
hscn_vl_* through the library, and the refusal of the three-relation resident launches -- all without a GPU."""
import ctypes

import pytest
import torch

VL_KEYS = ("att_src", "att_dst", "bias", "lin_src.weight", "lin_dst.weight")


def _model(vl="GAT", F=9, H=16, C=10, L=3):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L, vl_conv=vl)


def test_config_and_builder_defaults_are_the_reference():
    from graph_hscn.config.config import HSCNConfig
    from graph_hscn.model.hscn import build_hscn
    cfg = HSCNConfig("relu")
    assert cfg.vl_conv_type is None
    assert list(HSCNConfig.__dataclass_fields__)[-1] == "vl_conv_type"
    m = build_hscn(cfg, 9, 10)
    assert m.vl_conv is None
    assert sum(p.numel() for p in m.parameters()) == 3306
    assert not any("virtual__to__local" in k for k in m.state_dict())
    for conv in m.convs:
        assert list(conv.convs) == ["local__to__virtual", "local__to__local", "virtual__to__virtual"]
    m2 = build_hscn(HSCNConfig("relu", vl_conv_type="GAT"), 9, 10)
    assert m2.vl_conv == "GAT"


def test_state_dict_keys_and_parameter_count():
    m = _model()
    sd = m.state_dict()
    for l in range(3):
        for k in VL_KEYS:
            assert f"convs.{l}.convs.virtual__to__local.{k}" in sd
        assert list(m.convs[l].convs)[-1] == "virtual__to__local"
    assert sum(p.numel() for p in m.parameters()) == 4762
    assert sum(p.numel() for p in m.vl_params()) == 4762
    assert len({id(p) for p in m.vl_params()}) == len(list(m.parameters()))


def test_other_vl_conv_is_a_value_error():
    with pytest.raises(ValueError, match="GCN"):
        _model(vl="GCN")


def test_vl_envelope_answers_through_the_library():
    from graph_hscn import _hip
    from graph_hscn.loader.synthetic import make_dataset
    lib = _hip.lib()
    graphs = make_dataset("peptides_func", 64, seed=0)
    max_n = max(max(g.num_nodes for g in graphs), 444)
    max_e = max(max(g.edge_index.size(1) for g in graphs), 1000)
    assert lib.hscn_vl_supported(9, 16, 3, 10, max_n, 16, max_e, 136) == 1        # the full Peptides shape, K = 16
    assert lib.hscn_vl_supported(9, 32, 3, 10, 250, 16, 600, 136) == 1
    assert lib.hscn_vl_supported(9, 24, 3, 10, 444, 16, 1000, 136) == 0           # H must be 16 / 32
    assert lib.hscn_vl_supported(17, 16, 3, 10, 100, 16, 300, 136) == 0           # F <= H
    assert lib.hscn_vl_supported(9, 64, 3, 10, 100, 16, 300, 136) == 0
    assert lib.hscn_vl_supported(9, 16, 3, 10, 5000, 16, 10000, 136) == 0         # does not fit LDS
    assert lib.hscn_vl_param_count(9, 16, 3, 10) == 4762
    assert lib.hscn_vl_param_count(9, 16, 1, 10) == 6 * 16 * 9 + 8 * 16 + 256 + 16 + 160 + 10
    types = _hip._SIGNATURES["hscn_vl_train_step"][1]
    blank = [None if t is ctypes.c_void_p else 0 for t in types]
    assert lib.hscn_vl_train_step(*blank) == 0                                    # B = 0: nothing to do
    one = list(blank)
    one[15] = 1                                                                   # B = 1, target NULL
    assert types[15] is ctypes.c_int64 and lib.hscn_vl_train_step(*one) == -1     # HSCN_E_BADARG
    assert lib.hscn_vl_forward(*[None if t is ctypes.c_void_p else 0 for t in _hip._SIGNATURES["hscn_vl_forward"][1]]) == 0


def test_model_reasons_without_a_batch():
    assert _model().resident_reason() is None
    assert "H=64" in _model(H=64).resident_reason()
    assert "virtual" in _model(vl=None).resident_reason()


def test_three_relation_launches_refuse_the_vl_model_and_name_the_relation():
    from graph_hscn import engine
    from graph_hscn.engine import ResidentMeta
    from graph_hscn.step import ResidentTrainStep
    m = _model()
    name = r"\('virtual', 'to', 'local'\)"
    z = torch.zeros(2, dtype=torch.int32)
    meta = ResidentMeta(z, z, z, z, z, 1, 10, 4, 20, 10, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=name):
        engine.supported(9, 16, 3, 10, meta, torch.float32, model=m)
    with pytest.raises(RuntimeError, match=name):
        engine.supported(9, 16, 3, 10, meta, torch.float16, model=m)               # half storage
    with pytest.raises(RuntimeError, match=name):
        ResidentTrainStep(m, object(), "cross_entropy")
    with pytest.raises(RuntimeError, match=name):
        m._resident_params()
    m.engine = "resident"
    with pytest.raises(RuntimeError, match=name):
        m._resident_plan({}, {}, None)
    m.compute_virtual = False
    with pytest.raises(ValueError, match="compute_virtual"):
        m({}, {}, None)
    # the reference's model is untouched by the guard
    assert _model(vl=None)._resident_params() is not None
