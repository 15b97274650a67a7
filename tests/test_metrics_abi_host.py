"""The device-side evaluation surface without a GPU: the metric entry points of libhscn.so refuse bad arguments
before any launch, their workspace grows with the input, and the Python layer (``metrics.eval_ap_hip`` /
``eval_mae_hip``, ``train.eval_resident.DeviceEvaluator``, the keyword-only arguments of ``fit_resident``) is there
and refuses CPU tensors and contradictory arguments.  (tests/test_abi.py checks that header, binding and library
agree on the new symbol names.)"""
import ctypes
import inspect

import pytest
import torch

_BUF = ctypes.create_string_buffer(512)
_HERE = ctypes.addressof(_BUF)         # a host buffer standing in for pointers the checks only compare with NULL


def test_metric_entry_points_check_arguments_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert lib.hscn_average_precision(None, None, -1, 10, None, None, None, None, None, 0, None) == -1
    assert lib.hscn_mean_absolute_error(None, None, -1, 10, None, None, None) == -1
    here = [_HERE] * 2
    assert lib.hscn_average_precision(*here, 0, 10, _HERE, _HERE, _HERE, _HERE, _HERE, 1 << 20, None) == -1    # G < 1
    assert lib.hscn_average_precision(*here, 8, 0, _HERE, _HERE, _HERE, _HERE, _HERE, 1 << 20, None) == -1     # C < 1
    assert lib.hscn_average_precision(None, _HERE, 8, 2, _HERE, _HERE, _HERE, _HERE, _HERE, 1 << 20, None) == -1
    assert lib.hscn_average_precision(*here, 8, 2, _HERE, _HERE, _HERE, _HERE, None, 1 << 20, None) == -1
    assert lib.hscn_average_precision(*here, 8, 2, _HERE, _HERE, _HERE, _HERE, _HERE, 0, None) == -2           # workspace
    need = lib.hscn_average_precision_workspace_bytes(40000, 11)
    assert lib.hscn_average_precision(*here, 40000, 11, _HERE, _HERE, _HERE, _HERE, _HERE, need - 1, None) == -2
    assert lib.hscn_mean_absolute_error(*here, 0, 11, _HERE, _HERE, None) == -1
    assert lib.hscn_mean_absolute_error(*here, 8, 11, None, _HERE, None) == -1
    assert lib.hscn_mean_absolute_error(*here, 8, 11, _HERE, None, None) == -1


def test_average_precision_workspace_grows_with_the_input_and_is_small_while_the_keys_fit_lds():
    from graph_hscn import _hip
    ws = _hip.lib().hscn_average_precision_workspace_bytes
    sizes = (1, 2, 63, 64, 65, 1000, 2331, 10874, 16384, 16385, 40000, 100000)
    for C in (1, 10, 11, 64, 65):
        got = [ws(G, C) for G in sizes]
        assert got == sorted(got), (C, got)
        for G, b in zip(sizes, got):
            if G <= 16384:
                assert b <= 1024, (G, C, b)            # the per-class flag words only: the keys stay in LDS
            else:
                n2 = 1 << (G - 1).bit_length()
                assert b >= C * n2 * 8, (G, C, b)      # 8-byte keys of every class, padded to a power of two
    for G in sizes:
        got = [ws(G, C) for C in (1, 2, 10, 11, 64, 65, 200)]
        assert got == sorted(got), (G, got)


def test_hip_metrics_import_and_refuse_cpu_tensors():
    from graph_hscn.metrics import (average_precision_launch, eval_ap_hip, eval_mae_hip,
                                    mean_absolute_error_launch)
    y = (torch.rand(8, 3) < 0.5).float()
    s = torch.rand(8, 3)
    for fn in (eval_ap_hip, eval_mae_hip, average_precision_launch, mean_absolute_error_launch):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(y, s)
    with pytest.raises(ValueError):
        eval_ap_hip(y, s[:, :2])


def test_metric_value_applies_the_reference_error_behaviour():
    from graph_hscn.metrics import eval_ap, metric_value
    assert metric_value("ap", 0.25, 0) == 0.25 and metric_value("mae", 1.5, 0) == 1.5
    with pytest.raises(RuntimeError) as hip:
        metric_value("ap", 0.0, 1)
    with pytest.raises(RuntimeError) as ref:
        eval_ap(torch.ones(4, 2), torch.rand(4, 2))
    assert str(hip.value) == str(ref.value)
    with pytest.raises(ValueError, match="Input contains NaN."):
        metric_value("ap", 0.5, 2)
    with pytest.raises(Exception, match="Model is predicting NaN."):
        metric_value("mae", 0.5, 2)


def test_device_evaluator_imports_and_refuses_a_cpu_model():
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.train.eval_resident import DeviceEvaluator
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3)
    with pytest.raises(ValueError):
        DeviceEvaluator([object()], model, "cross_entropy", 4, metric="auroc")
    with pytest.raises(RuntimeError, match="cuda"):
        DeviceEvaluator([object()], model, "cross_entropy", 4, metric="ap")


def test_fit_resident_takes_the_evaluation_arguments_keyword_only():
    from graph_hscn.train.train_resident import fit_resident
    params = inspect.signature(fit_resident).parameters
    for name in ("eval_graphs", "metric", "eval_history"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None, name
    for name in ("eval_loaders", "metric_fn", "seed", "reducer", "flat_optimizer", "epoch_orders"):
        assert params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name


def test_fit_resident_refuses_metric_and_metric_fn_together_before_touching_a_device():
    """The check sits ahead of the device check: a CPU model (which fit_resident refuses with a RuntimeError) still
    gets the ValueError."""
    from graph_hscn.config.config import ACT_DICT, OptimConfig, TrainingConfig
    from graph_hscn.metrics import eval_ap
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.train.train_resident import fit_resident
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3)
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=1, eval_period=1, patience=1)
    cfg = OptimConfig("adamW", lr=0.01)
    with pytest.raises(ValueError, match="not both"):
        fit_resident(None, cfg, tc, [], None, model, batch_size=4, metric="ap", metric_fn=eval_ap)
    with pytest.raises(ValueError):
        fit_resident(None, cfg, tc, [], None, model, batch_size=4, metric="auroc")
    with pytest.raises(RuntimeError, match="cuda"):
        fit_resident(None, cfg, tc, [], None, model, batch_size=4, metric="ap")
