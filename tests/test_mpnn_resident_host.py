"""Host-side surface of the MPNN baseline's one-launch kernels (include/hscn.h, ABI 20): the envelope query, the
parameter count and the model's engine switch -- no GPU needed."""
import pytest
import torch


def _lib():
    from graph_hscn import _hip
    return _hip.lib()


def test_param_count_is_the_models():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    for F, H, C, L in ((9, 16, 10, 3), (9, 16, 11, 2), (16, 32, 10, 5)):
        m = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], F, H, C, L)
        assert _lib().hscn_mpnn_param_count(F, H, L, C) == sum(p.numel() for p in m.parameters())


def test_supported_envelope():
    lib = _lib()
    assert lib.hscn_mpnn_supported(9, 16, 3, 10, 444, 2664) == 1        # Peptides' largest graph at H = 16
    assert lib.hscn_mpnn_supported(9, 16, 3, 11, 444, 2664) == 1
    assert lib.hscn_mpnn_supported(9, 32, 3, 10, 150, 900) == 1
    assert lib.hscn_mpnn_supported(17, 16, 3, 10, 444, 2664) == 0       # F > H
    assert lib.hscn_mpnn_supported(9, 24, 3, 10, 100, 600) == 0         # H not in {16, 32}
    assert lib.hscn_mpnn_supported(9, 16, 3, 17, 100, 600) == 0         # C > H
    assert lib.hscn_mpnn_supported(9, 16, 1, 10, 100, 600) == 0         # one convolution
    assert lib.hscn_mpnn_supported(1433, 16, 2, 7, 2708, 10556) == 0    # Cora's shape stays layered
    assert lib.hscn_mpnn_supported(9, 16, 3, 10, 3000, 9000) == 0       # over 160 KB of LDS


def test_engine_default_and_model_envelope():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.nn.conv import GATConv
    gcn, relu = CONV_DICT["gcn"], ACT_DICT["relu"]
    m = MPNN(gcn, relu, 9, 16, 10, 3, 0.2)
    assert m.engine == "layered"
    assert m.supported() and m.resident_reason() is None
    for act in ("elu", "identity", "tanh"):
        assert MPNN(gcn, ACT_DICT[act], 9, 16, 10, 3).supported()
    assert "normalisation" in MPNN(gcn, relu, 9, 16, 10, 3, use_layer_norm=True).resident_reason()
    assert "GATConv" in MPNN(lambda i, o: GATConv(i, o, add_self_loops=False), relu, 9, 16, 10, 3).resident_reason()
    assert not MPNN(gcn, relu, 20, 16, 10, 3).supported()


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib()
    # a NULL pointer table / NULL targets: HSCN_E_BADARG, no launch
    assert lib.hscn_mpnn_train_step(None, None, 0, None, None, 0, 1, 9, 16, 3, 10, 1, None, 10, 10, None, 0, 0.1,
                                    None, None, None, None, None, 0.0, 0, None, 0, None) == -1
    assert lib.hscn_mpnn_forward(None, None, 0, None, None, 0, 1, 9, 16, 3, 10, 1, None, 10, 10, None, 0, 0.1,
                                 None, None, None, None, None, None) == -1
