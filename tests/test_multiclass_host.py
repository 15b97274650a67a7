"""Class-index targets, host side: the torch definitions of accuracy and macro-F1 against scikit-learn, the
criterion's CPU branch, the binding's new symbols and the metric plumbing.  No GPU."""
import pytest
import torch
import sklearn.metrics as sk
import torch.nn.functional as F


def _cases():
    g = torch.Generator().manual_seed(7)
    cases = {}
    for G, C in ((1, 3), (37, 2), (64, 10), (301, 64)):
        s = torch.randn(G, C, generator=g)
        s[::3, 0] = s[::3].max(1).values                      # tied maxima: column 0 and the row's own maximum
        if C > 2:
            s[1::5, 1] = s[1::5, 2] = s[1::5].max(1).values + 1.0     # two maximal columns, neither the first column
        cases[f"random_G{G}_C{C}"] = (torch.randint(0, C, (G,), generator=g), s)
    y = torch.randint(0, 3, (50,), generator=g)
    s = torch.randn(50, 5, generator=g)
    s[:, 3:] = -1e3                                            # classes 3, 4: never true, never predicted
    cases["absent_class"] = (y, s)
    s = torch.randn(50, 4, generator=g)
    s[:7, 3] = 1e3                                             # class 3 is predicted but never true
    cases["predicted_never_true"] = (torch.randint(0, 3, (50,), generator=g), s)
    s = torch.zeros(20, 4)
    s[:, 2] = 1.0
    cases["all_one_class"] = (torch.full((20,), 2, dtype=torch.int64), s)
    cases["all_tied"] = (torch.randint(0, 4, (20,), generator=g), torch.zeros(20, 4))
    return cases


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_and_macro_f1_are_sklearns(name):
    from graph_hscn.metrics import confusion_matrix, eval_accuracy, eval_f1_macro
    y, s = CASES[name]
    pred = s.numpy().argmax(1)                                 # numpy: the first maximal column
    assert abs(eval_accuracy(y, s) - sk.accuracy_score(y.numpy(), pred)) <= 1e-12
    assert abs(eval_f1_macro(y, s) - sk.f1_score(y.numpy(), pred, average="macro")) <= 1e-12
    C = s.size(1)
    want = sk.confusion_matrix(y.numpy(), pred, labels=list(range(C)))
    assert torch.equal(confusion_matrix(y, s), torch.from_numpy(want))


def test_metric_definitions_refuse_what_they_cannot_mean():
    from graph_hscn.metrics import eval_accuracy, eval_f1_macro
    s = torch.zeros(4, 3)
    with pytest.raises(IndexError):
        eval_accuracy(torch.tensor([0, 1, 3, 0]), s)
    with pytest.raises(IndexError):
        eval_f1_macro(torch.tensor([0, -1, 2, 0]), s)
    with pytest.raises(TypeError):
        eval_accuracy(torch.zeros(4), s)
    with pytest.raises(ValueError, match="NaN"):
        eval_accuracy(torch.zeros(4, dtype=torch.int64), torch.full((4, 3), float("nan")))


def test_criterion_on_cpu_tensors_is_the_torch_expression():
    from graph_hscn.loss import criterion
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(9, 5, generator=g, requires_grad=True)
    true = torch.randint(0, 5, (9,), generator=g)
    loss, score = criterion("cross_entropy", pred, true)
    want_score = F.log_softmax(pred, dim=-1)
    assert torch.equal(score, want_score) and torch.equal(loss, F.nll_loss(want_score, true))
    (g_got,) = torch.autograd.grad(loss, pred)
    (g_want,) = torch.autograd.grad(F.nll_loss(F.log_softmax(pred, dim=-1), true), pred)
    assert torch.equal(g_got, g_want)
    with pytest.raises(IndexError):
        criterion("cross_entropy", pred, torch.full((9,), 5))
    # the multilabel branch on the CPU, unchanged
    y = (torch.rand(9, 5, generator=g) < 0.5).float()
    loss, score = criterion("cross_entropy", pred, y)
    assert torch.equal(loss, F.binary_cross_entropy_with_logits(pred, y)) and torch.equal(score, torch.sigmoid(pred))


def test_binding_declares_the_new_symbols():
    from graph_hscn import _hip
    sig = _hip._SIGNATURES
    for name in ("hscn_softmax_nll_fwd", "hscn_softmax_nll_workspace_bytes", "hscn_multiclass_metrics"):
        assert name in sig and name in _hip.exported_symbols()
    assert len(sig["hscn_softmax_nll_fwd"][1]) == 11 and len(sig["hscn_multiclass_metrics"][1]) == 9
    assert _hip.ABI_VERSION == 24
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "hscn.h")).read()
    for name in ("hscn_softmax_nll_fwd(", "hscn_softmax_nll_workspace_bytes(", "hscn_multiclass_metrics("):
        assert name in header


def test_metric_value_passes_the_class_metrics_through_and_maps_the_flags():
    from graph_hscn import metrics as M
    assert M.metric_value("accuracy", 0.25, 0) == 0.25 and M.metric_value("f1_macro", 0.5, 0) == 0.5
    assert M.result_index("accuracy") == 0 and M.result_index("f1_macro") == 1
    assert M.result_index("ap") == 0 and M.result_index("mae") == 0
    for name in M.CLASS_METRICS:
        with pytest.raises(ValueError, match="NaN"):
            M.metric_value(name, 0.0, M.NAN_INPUT)
        with pytest.raises(IndexError):
            M.metric_value(name, 0.0, M.TARGET_OUT_OF_RANGE)
        assert M.metric_launch(name) is M.multiclass_metrics_launch
    assert M.eval_hip("accuracy") is M.eval_accuracy_hip and M.eval_hip("f1_macro") is M.eval_f1_macro_hip
    with pytest.raises(ValueError):
        M.metric_buffers("auc", 4, 3, "cpu")
    out = M.metric_buffers("f1_macro", 4, 3, "cpu")           # (allocation needs no device)
    assert out.ap.shape == (3,) and out.valid.shape == (3, 3) and out.valid.dtype == torch.int32
    assert out.workspace is None and out.packed.numel() == 32


def test_argument_checks_of_the_new_calls_without_a_gpu():
    """Refused before any launch: no device is touched."""
    import ctypes
    from graph_hscn import _hip
    L = _hip.lib()                                   # raises if the .so or a declared symbol is missing: no fallback
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    E_BADARG, E_WORKSPACE = -1, -2
    nll = L.hscn_softmax_nll_fwd
    assert nll(p, p, 0, 4, p, None, p, p, None, 0, None) == E_BADARG          # R < 1
    assert nll(p, p, 4, 0, p, None, p, p, None, 0, None) == E_BADARG          # C < 1
    assert nll(p, p, 4, 1025, p, None, p, p, None, 0, None) == E_BADARG       # C above the cap
    assert nll(p, p, 4, 4, None, None, p, p, None, 0, None) == E_BADARG       # NULL loss
    assert nll(p, p, 4, 4, p, None, None, p, None, 0, None) == E_BADARG       # NULL grad
    assert nll(p, p, 4, 4, p, None, p, None, None, 0, None) == E_BADARG       # NULL flags
    assert nll(p, p, 257, 4, p, None, p, p, None, 0, None) == E_BADARG        # two workgroups, no workspace
    assert nll(p, p, 257, 4, p, None, p, p, p, 4, None) == E_WORKSPACE
    ws = L.hscn_softmax_nll_workspace_bytes
    assert (ws(1, 10), ws(256, 10), ws(257, 10), ws(1000, 64), ws(4, 1025), ws(0, 4)) == (0, 0, 8, 16, 0, 0)
    mc = L.hscn_multiclass_metrics
    assert mc(p, p, 0, 4, p, p, p, p, None) == E_BADARG
    assert mc(p, p, 4, 129, p, p, p, p, None) == E_BADARG
    assert mc(p, p, 4, 4, None, p, p, p, None) == E_BADARG
    assert mc(p, p, 4, 4, p, p, None, p, None) == E_BADARG


def test_batching_tells_class_indices_from_label_rows():
    from graph_hscn.train import batching
    assert batching.class_index_targets(torch.zeros(4, dtype=torch.int64))
    assert not batching.class_index_targets(torch.zeros(4, 3)) and not batching.class_index_targets(None)
    assert not batching.class_index_targets(torch.zeros(4))
    assert batching.score_width(object(), torch.zeros(4, 3)) == 3
    with pytest.raises(ValueError, match="HSCN"):
        batching.score_width(object(), torch.zeros(4, dtype=torch.int64))
