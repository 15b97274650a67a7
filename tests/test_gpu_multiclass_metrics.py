"""hscn_multiclass_metrics (csrc/metrics.hip): the confusion matrix bit for bit against a host-built one, accuracy
and macro-F1 against scikit-learn to 1e-12, the flags, and the ``out=`` form."""
import pytest
import sklearn.metrics as sk
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(G, C, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(G, C, generator=g)
    s[::3, 0] = s[::3].max(1).values                               # tied maxima: the first column wins
    if C > 2:
        s[1::5, 1] = s[1::5, 2] = s[1::5].max(1).values + 1.0       # two maximal columns, neither the first
    s[2::7] = 0.0                                                  # a whole row tied
    return torch.randint(0, C, (G,), generator=g), s


def _host(y, s):
    C = s.size(1)
    pred = s.numpy().argmax(1)
    conf = torch.from_numpy(sk.confusion_matrix(y.numpy(), pred, labels=list(range(C)))).to(torch.int32)
    return conf, sk.accuracy_score(y.numpy(), pred), sk.f1_score(y.numpy(), pred, average="macro"), \
        sk.f1_score(y.numpy(), pred, average=None, labels=list(range(C)), zero_division=0)


def _check(y, s):
    from graph_hscn import metrics as M
    out = M.multiclass_metrics_launch(y.to(DEV), s.to(DEV))
    conf, acc, f1, per_class = _host(y, s)
    assert torch.equal(out.valid.cpu(), conf)
    assert int(out.flags.item()) == 0
    assert abs(float(out.result[0]) - acc) <= 1e-12 and abs(float(out.result[1]) - f1) <= 1e-12
    assert float((out.ap.cpu() - torch.from_numpy(per_class)).abs().max()) <= 1e-12
    assert abs(M.eval_accuracy_hip(y.to(DEV), s.to(DEV)) - acc) <= 1e-12
    assert abs(M.eval_f1_macro_hip(y.to(DEV), s.to(DEV)) - f1) <= 1e-12
    # the torch definitions, where the tensors live
    assert abs(M.eval_accuracy(y.to(DEV), s.to(DEV)) - acc) <= 1e-12
    assert abs(M.eval_f1_macro(y.to(DEV), s.to(DEV)) - f1) <= 1e-12
    return out


@pytest.mark.parametrize("C", [2, 10, 64])
@pytest.mark.parametrize("G", [1, 64, 65, 5000])
def test_confusion_accuracy_and_f1(G, C):
    _check(*_case(G, C, 100 * C + G))


def test_more_rows_than_one_pass_of_the_grid_and_the_widest_matrix():
    _check(*_case(256 * 256 + 77, 3, 5))            # every workgroup takes a second, partial pass
    _check(*_case(700, 128, 6))                     # C at the cap: 64 KB of LDS


def test_absent_classes_and_a_single_class():
    g = torch.Generator().manual_seed(9)
    s = torch.randn(90, 6, generator=g)
    s[:, 4:] = -1e3                                 # classes 4, 5: never true, never predicted
    s[:11, 3] = 1e3                                 # class 3: predicted, never true
    out = _check(torch.randint(0, 3, (90,), generator=g), s)
    assert float(out.ap[4]) == 0.0 and float(out.ap[3]) == 0.0
    s = torch.zeros(33, 4)
    s[:, 2] = 1.0
    out = _check(torch.full((33,), 2, dtype=torch.int64), s)
    assert float(out.result[0]) == 1.0 and float(out.result[1]) == 1.0


def test_flags_reach_the_host_as_the_references_errors():
    from graph_hscn import metrics as M
    y, s = _case(100, 5, 3)
    s[41, 2] = float("nan")
    out = M.multiclass_metrics_launch(y.to(DEV), s.to(DEV))
    f64, i32 = M.read_packed(out.packed)
    assert int(i32[0]) == M.NAN_INPUT
    for name in M.CLASS_METRICS:
        with pytest.raises(ValueError, match="NaN"):
            M.metric_value(name, float(f64[M.result_index(name)]), int(i32[0]))
    with pytest.raises(ValueError, match="NaN"):
        M.eval_accuracy_hip(y.to(DEV), s.to(DEV))
    y, s = _case(100, 5, 4)
    bad = y.clone()
    bad[7], bad[99] = 5, -1
    out = M.multiclass_metrics_launch(bad.to(DEV), s.to(DEV))
    assert int(out.flags.item()) == M.TARGET_OUT_OF_RANGE
    keep = torch.ones(100, dtype=torch.bool)
    keep[7] = keep[99] = False
    assert torch.equal(out.valid.cpu(), _host(y[keep], s[keep])[0])       # the other rows, nothing out of bounds
    with pytest.raises(IndexError):
        M.eval_f1_macro_hip(bad.to(DEV), s.to(DEV))
    with pytest.raises(RuntimeError, match="device tensors only"):
        M.multiclass_metrics_launch(y, s)
    # a non-contiguous device score (a column slice) is made contiguous, not refused
    wide = torch.cat([s, s], 1).to(DEV)
    out = M.multiclass_metrics_launch(y.to(DEV), wide[:, :5])
    assert torch.equal(out.valid.cpu(), _host(y, s)[0])


def test_out_form_launches_again_into_the_same_buffers_without_allocating():
    from graph_hscn import metrics as M
    y1, s1 = _case(300, 10, 1)
    y2, s2 = _case(300, 10, 2)
    y1, s1, y2, s2 = (t.to(DEV) for t in (y1, s1, y2, s2))
    out = M.metric_buffers("accuracy", 300, 10, DEV)
    M.multiclass_metrics_launch(y1, s1, out=out)
    first = (out.valid.clone(), out.result.clone())
    ptrs = [t.data_ptr() for t in (out.result, out.flags, out.ap, out.valid, out.packed)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    again = M.multiclass_metrics_launch(y2, s2, out=out)
    again = M.multiclass_metrics_launch(y1, s1, out=again)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again is out and ptrs == [t.data_ptr() for t in (out.result, out.flags, out.ap, out.valid, out.packed)]
    assert torch.equal(out.valid, first[0]) and torch.equal(out.result, first[1])     # rewritten, not added to
    with pytest.raises(ValueError, match="another shape"):
        M.multiclass_metrics_launch(y1, s1[:, :9].contiguous(), out=out)
