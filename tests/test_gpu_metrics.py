"""The HIP epoch metrics (csrc/metrics.hip: hscn_average_precision, hscn_mean_absolute_error) against the torch
restatements ``metrics.eval_ap`` / ``eval_mae`` evaluated on CPU float64 copies of the same tensors (``eval_ap`` is
itself pinned to sklearn by tests/test_host_logic.py), and against sklearn directly where it imports.

The bounds are a priori.  AP of a class: both sides add at most G non-negative float64 terms
(recall_run - recall_prev) * precision_run whose partial sums stay <= 1; every term is the same on both sides (the
same integer tp, P and n divided and multiplied in float64), so the two results differ only by the order of the
additions: each is within (G - 1) 2^-53 of the exact sum of the terms, |delta| <= 2 G 2^-53, and the asserted bound is
8 G 2^-53.  The mean adds C <= 11 such numbers and divides once.  ``valid`` must be equal exactly.
MAE: a float64 mean of G C non-negative terms, each an exact difference of two float32 values rounded once; any
summation order is within (G C - 1) 2^-53 of the exact sum, relatively; the bound is (G C + 2) 2^-53 relative."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53

# 4096 / 4097: 32 KB / 64 KB of keys in LDS beside the kernel's 16 KB of static scratch -- the last size a launch gets
# unasked and the first that has to opt in, and the only step at which the static part decides
SIZES = (2, 63, 64, 65, 1000, 2331, 4096, 4097, 10874, 16384, 16385, 40000)
CLASSES = (1, 10, 11)
KINDS = ("continuous", "quantised", "equal", "special", "nan_labels", "single_label_columns")


def _case(kind, G, C, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(G, C, generator=g) < 0.3).float()
    y[0], y[1] = 1.0, 0.0                           # every column holds both labels (G >= 2) unless the case says not
    s = torch.randn(G, C, generator=g)
    if kind == "quantised":
        s = torch.floor(torch.rand(G, C, generator=g) * 8) / 8          # 8 levels: long tie runs
    elif kind == "equal":
        s = torch.full((G, C), 0.25)
    elif kind == "special":
        pool = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-45, -1e-45, 3e-39, -3e-39, 1.0, -1.0, 1e-38])
        s = pool[torch.randint(0, pool.numel(), (G, C), generator=g)]
    elif kind == "nan_labels":
        drop = torch.rand(G, C, generator=g) < 0.1
        drop[:2] = False
        y[drop] = float("nan")
    elif kind == "single_label_columns":
        y[:, 0] = 1.0
        if C > 2:
            y[:, 2] = 0.0
            nan = torch.rand(G, generator=g) < 0.5
            y[nan, 2] = float("nan")                # zeros and NaN only: still a single label value
    return y, s


def _reference(y, s):
    """Per-class AP, validity and the mean through metrics._ap_one / eval_ap on CPU float64."""
    from graph_hscn.metrics import _ap_one, eval_ap
    y64, s64 = y.double(), s.double()
    ap, valid = [], []
    for c in range(y.shape[1]):
        col = y64[:, c]
        ok = bool((col == 1).any()) and bool((col == 0).any())
        valid.append(int(ok))
        lab = col == col
        ap.append(float(_ap_one(col[lab], s64[lab, c])) if ok else 0.0)
    mean = eval_ap(y, s) if any(valid) else None
    return ap, valid, mean


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("G", SIZES)
def test_average_precision_against_the_float64_restatement(G, C):
    from graph_hscn.metrics import average_precision_launch, eval_ap_hip
    for k, kind in enumerate(KINDS):
        if kind == "single_label_columns" and C == 1:
            continue                                # (C = 1 with its only column single-label: the error test below)
        y, s = _case(kind, G, C, seed=1000 * k + 7 * G + C)
        ap, valid, mean = _reference(y, s)
        yd, sd = y.to(DEV), s.to(DEV)
        out = average_precision_launch(yd, sd)
        got_ap, got_valid = out.ap.cpu().tolist(), out.valid.cpu().tolist()
        got_mean, got_n = out.result.cpu().tolist()
        flags = int(out.flags.cpu()[0])
        bound = 8 * G * U
        worst = max([abs(a - b) for a, b, v in zip(got_ap, ap, valid) if v] + [0.0])
        print(f"{kind} G={G} C={C}: max |dAP| {worst:.3e}, |dmean| {abs(got_mean - mean):.3e}, bound {bound:.3e}")
        assert got_valid == valid, (kind, got_valid, valid)
        assert got_n == sum(valid) and flags == 0
        for c in range(C):
            if valid[c]:
                assert abs(got_ap[c] - ap[c]) <= bound, (kind, c, got_ap[c], ap[c])
        assert abs(got_mean - mean) <= bound, (kind, got_mean, mean)
        assert abs(eval_ap_hip(yd, sd) - mean) <= bound
        again = average_precision_launch(yd, sd)                     # the same bits from a second call
        assert torch.equal(again.ap.view(torch.int64), out.ap.view(torch.int64))
        assert torch.equal(again.result.view(torch.int64), out.result.view(torch.int64))
        assert torch.equal(again.valid, out.valid)


@pytest.mark.parametrize("G,C", [(2, 1), (65, 10), (2331, 10), (10874, 10), (16385, 11), (40000, 1)])
def test_average_precision_against_sklearn(G, C):
    sk = pytest.importorskip("sklearn.metrics")
    from graph_hscn.metrics import average_precision_launch
    for k, kind in enumerate(("continuous", "quantised", "equal")):      # (sklearn refuses infinite scores)
        y, s = _case(kind, G, C, seed=50 * k + G + C)
        out = average_precision_launch(y.to(DEV), s.to(DEV))
        got = out.ap.cpu().tolist()
        for c in range(C):
            want = float(sk.average_precision_score(y[:, c].numpy(), s[:, c].double().numpy()))
            assert abs(got[c] - want) <= 8 * G * U, (kind, c, got[c], want)


def test_average_precision_errors():
    from graph_hscn.metrics import average_precision_launch, eval_ap, eval_ap_hip
    y, s = _case("continuous", 500, 10, seed=3)
    y1 = y.clone()
    y1[:, ::2], y1[:, 1::2] = 1.0, 0.0              # every column single-label
    with pytest.raises(RuntimeError) as ref:
        eval_ap(y1, s)
    with pytest.raises(RuntimeError) as hip:
        eval_ap_hip(y1.to(DEV), s.to(DEV))
    assert str(hip.value) == str(ref.value) and "No positively labeled data" in str(hip.value)
    s1 = s.clone()
    s1[17, 4] = float("nan")
    with pytest.raises(ValueError, match="Input contains NaN."):
        eval_ap_hip(y.to(DEV), s1.to(DEV))
    y2 = y.clone()
    y2[17, 4] = float("nan")                        # the NaN score sits in an unlabelled row: ignored with the row
    assert abs(eval_ap_hip(y2.to(DEV), s1.to(DEV)) - eval_ap(y2, torch.nan_to_num(s1))) <= 8 * 500 * U
    out = average_precision_launch(y.to(DEV), s.to(DEV))
    with pytest.raises(ValueError):
        average_precision_launch(y[:, :3].to(DEV), s[:, :3].to(DEV), out=out)


@pytest.mark.parametrize("C", (1, 11))
@pytest.mark.parametrize("G", SIZES)
def test_mean_absolute_error_against_the_float64_restatement(G, C):
    from graph_hscn.metrics import eval_mae, eval_mae_hip, mean_absolute_error_launch
    g = torch.Generator().manual_seed(G * 13 + C)
    y = torch.randn(G, C, generator=g) * 3
    p = torch.sigmoid(torch.randn(G, C, generator=g))
    want = eval_mae(y, p)
    yd, pd = y.to(DEV), p.to(DEV)
    out = mean_absolute_error_launch(yd, pd)
    got, count = out.result.cpu().tolist()
    rel = abs(got - want) / want
    print(f"MAE G={G} C={C}: relative error {rel:.3e}, bound {(G * C + 2) * U:.3e}")
    assert count == G * C and int(out.flags.cpu()[0]) == 0
    assert rel <= (G * C + 2) * U
    assert eval_mae_hip(yd, pd) == got
    again = mean_absolute_error_launch(yd, pd)
    assert torch.equal(again.result.view(torch.int64), out.result.view(torch.int64))
    pd[G // 2, C - 1] = float("nan")
    with pytest.raises(Exception, match="Model is predicting NaN."):
        eval_mae_hip(yd, pd)
