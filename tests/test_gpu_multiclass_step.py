"""Class-index targets through the device fast path: ``step.ResidentTrainStep`` as forward launch +
``hscn_softmax_nll_fwd`` + backward launch, its capture, ``fit_resident`` and ``DeviceEvaluator``.

Tolerances are tests/test_gpu_step.py's: the launch pair against the autograd path on the same engine is bit for bit
(``torch.equal``: the same launches with the same arguments); against another grouping of the same sums (here the
layered operators) that file's ``pool_order_close`` (1e-5 of the tensor's magnitude) for outputs and
``grads_close(rel=1e-5)`` for gradients.  Half storage against the float32 twin: tests/test_gpu_f16.py's
construction, |pred16 - pred32| <= u (G + ... + G^L) scale with u = 2^-11, G = 2; a log-softmax moves by at most twice
the largest move of its inputs (|d max| + |d logsumexp|), and the mean NLL by no more than its terms.  A parameter
gradient is a sum of products (stored activation) x (upstream gradient): both factors carry at most that relative
error, so |g16 - g32| <= 2 u (G + ... + G^L) max|g32| to first order.  The hand-off of ``g_pred`` under half storage
is checked exactly: the half-storage step equals the autograd path on the same half batch bit for bit."""
import numpy as np
import pytest
import torch

from tests.helpers import grads_close, pool_order_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = 8


def _graphs(n, C, seed):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    rng = np.random.default_rng(seed)
    graphs = make_dataset("peptides_func", n, seed=seed)
    for g in graphs:
        g.y = torch.tensor([int(rng.integers(0, C))])
    return [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]


def _batch(n, C, seed):
    from graph_hscn.data import HeteroBatch
    hb = HeteroBatch.from_data_list(_graphs(n, C, seed))
    y = hb["local"].y
    assert y.dtype == torch.int64 and tuple(y.shape) == (n,)
    return hb


def _model(C, H=16, L=3, seed=0):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(seed)
    m = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, H, C, L).to(DEV)
    m.engine = "resident"
    return m


def _autograd(model, d, engine):
    from graph_hscn.loss import criterion
    keep, model.engine = model.engine, engine
    try:
        model.zero_grad(set_to_none=True)
        pred = model(d.x_dict, d.edge_index_dict, d)
        assert model.last_engine == engine
        loss, score = criterion("cross_entropy", pred, d["local"].y)
        loss.backward()
    finally:
        model.engine = keep
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    none = {n for n, p in model.named_parameters() if p.grad is None}
    return pred.detach(), loss.detach(), score.detach(), grads, none


@pytest.mark.parametrize("B,L,C,H", [(6, 1, 3, 16), (7, 3, 10, 16), (1, 3, 16, 16), (1, 3, 10, 32), (5, 3, 10, 32)])
def test_step_runs_and_agrees_with_both_autograd_paths(B, L, C, H):
    from graph_hscn.step import ResidentTrainStep
    d = _batch(B, C, seed=10 * B + C).to(DEV)
    model = _model(C, H, L)
    rs = ResidentTrainStep(model, d, "cross_entropy")          # (TypeError on float-only steps: the feature)
    assert rs.class_index and rs.one_launch is False and rs.score.shape == (B, C)
    rs.bind_grads()
    rs.run()
    rs.run()                                                   # idempotent: buffers are rewritten
    torch.cuda.synchronize()
    rs.check()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    got_none = {n for n, p in model.named_parameters() if p.grad is None}
    pred, loss, score = rs.pred.clone(), rs.loss.clone(), rs.score.clone()
    assert got_none and all(".convs." in n for n in got_none)  # the virtual branch: the prediction does not reach it
    # the same forward launch as the BCE pair's
    y_f = (torch.rand(B, C, generator=torch.Generator().manual_seed(1)) < 0.3).float().to(DEV)
    pair = ResidentTrainStep(model, d, "cross_entropy", target=y_f, one_launch=False)
    pair.run()
    assert torch.equal(pair.pred, pred)
    # the autograd path on the same engine: the same three launches
    a_pred, a_loss, a_score, a_grads, a_none = _autograd(model, d, "resident")
    assert torch.equal(a_pred, pred) and torch.equal(a_loss, loss) and torch.equal(a_score, score)
    assert a_none == got_none and a_grads.keys() == got.keys()
    for n in got:
        assert torch.equal(a_grads[n], got[n]), n
    # the layered operators
    l_pred, l_loss, l_score, l_grads, l_none = _autograd(model, d, "layered")
    assert pool_order_close(pred, l_pred) and pool_order_close(score, l_score) and pool_order_close(loss, l_loss)
    assert l_none == got_none and l_grads.keys() == got.keys()
    for n in got:
        assert grads_close(got[n], l_grads[n], rel=1e-5), n
    # float64 on the host from the step's own prediction: the criterion launch in place
    import torch.nn.functional as F
    x = pred.cpu().double()
    logp64 = F.log_softmax(x, -1)
    assert float((score.cpu().double() - logp64).abs().max()) <= 1e-5
    assert abs(float(loss) - float(F.nll_loss(logp64, d["local"].y.cpu()))) <= 1e-5


def test_accumulate_adds_two_runs_in_order():
    from graph_hscn.step import ResidentTrainStep
    C = 10
    d1, d2 = _batch(5, C, 1).to(DEV), _batch(5, C, 2).to(DEV)
    model = _model(C)
    singles = []
    for d in (d1, d2):
        s = ResidentTrainStep(model, d, "cross_entropy")
        s.run()
        singles.append((s.grads[:s.P].clone(), s.loss.clone()))
    first = ResidentTrainStep(model, d1, "cross_entropy", accumulate=True)
    first.run()
    torch.cuda.synchronize()
    assert torch.equal(first.grads[:first.P], singles[0][0])               # (onto zeros)
    # the second batch's step folds onto what the first one left
    second = ResidentTrainStep(model, d2, "cross_entropy", accumulate=True)
    second.grads.copy_(first.grads)
    second.run()
    torch.cuda.synchronize()
    assert torch.equal(second.grads[:second.P], singles[0][0] + singles[1][0])
    assert torch.equal(second.loss, singles[1][1])                         # the loss of the last run
    second.run()
    torch.cuda.synchronize()
    assert torch.equal(second.grads[:second.P], (singles[0][0] + singles[1][0]) + singles[1][0])


def test_refusals():
    from graph_hscn.step import ResidentTrainStep
    C = 10
    d = _batch(4, C, 3).to(DEV)
    model = _model(C)
    with pytest.raises(RuntimeError, match="no class-index loss row"):
        ResidentTrainStep(model, d, "cross_entropy", one_launch=True)
    with pytest.raises(TypeError):
        ResidentTrainStep(model, d, "l1")                                  # class indices are no L1 target
    with pytest.raises(TypeError):
        ResidentTrainStep(model, d, "cross_entropy", target=d["local"].y.to(torch.int32))
    with pytest.raises(ValueError):
        ResidentTrainStep(model, d, "cross_entropy", target=d["local"].y[:3].contiguous())
    bad = d["local"].y.clone()
    bad[1] = C
    rs = ResidentTrainStep(model, d, "cross_entropy", target=bad)
    rs.run()
    with pytest.raises(IndexError):
        rs.check()
    rs.check()                                                             # (read and cleared)


def test_other_models_refuse_class_indices_as_before():
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.nn.conv import GCNConv
    from graph_hscn.step import MPNNResidentTrainStep, VLResidentTrainStep
    C = 10
    graphs = make_dataset("peptides_func", 4, seed=5)
    for i, g in enumerate(graphs):
        g.y = torch.tensor([i % C])
    b = Batch.from_data_list(graphs).to(DEV)
    b.x = b.x.float()
    mp = MPNN(GCNConv, ACT_DICT["relu"], 9, 16, C, 3).to(DEV)
    reason = mp.resident_reason(b)
    assert isinstance(reason, str) and "class-index" in reason and not mp.supported(b)
    with pytest.raises(RuntimeError, match="class-index"):
        MPNNResidentTrainStep(mp, b, "cross_entropy")
    d = _batch(4, C, 6).to(DEV)
    torch.manual_seed(0)
    vl = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, C, 3, vl_conv="GAT").to(DEV)
    assert vl.resident_reason(d) == ("class-index (multiclass) targets: the fused loss row takes [B, C] multilabel / "
                                     "regression targets")
    with pytest.raises(RuntimeError, match="class-index"):
        VLResidentTrainStep(vl, d, "cross_entropy")


def test_half_storage_step_against_its_float32_twin():
    from graph_hscn.step import ResidentTrainStep
    C, L = 10, 3
    d32 = _batch(6, C, 8).to(DEV)
    d16 = d32.with_feature_dtype(torch.float16)
    assert torch.equal(d16["local"].x.float(), d32["local"].x)
    model = _model(C, 16, L)
    s32 = ResidentTrainStep(model, d32, "cross_entropy")
    s16 = ResidentTrainStep(model, d16, "cross_entropy")
    s32.run()
    s16.run()
    torch.cuda.synchronize()
    s16.check()
    U = 2.0 ** -11
    gain = sum(2.0 ** l for l in range(1, L + 1))
    ps = max(1.0, float(s32.pred.abs().max()))
    d_pred = float((s16.pred - s32.pred).abs().max())
    d_score = float((s16.score - s32.score).abs().max())
    d_loss = abs(float(s16.loss) - float(s32.loss))
    print(f"[f16 class-index] |dpred| {d_pred:.3e} (bound {U * gain * ps:.3e})  |dscore| {d_score:.3e}  "
          f"|dloss| {d_loss:.3e} (bound {2 * U * gain * ps:.3e})")
    assert d_pred <= U * gain * ps
    assert d_score <= 2 * U * gain * ps and d_loss <= 2 * U * gain * ps
    for (p, g16), (_, g32) in zip(s16.param_grads, s32.param_grads):
        gs = max(1e-3, float(g32.abs().max()))
        d_g = float((g16 - g32).abs().max())
        print(f"[f16 class-index] grad {tuple(p.shape)}: |dg| {d_g:.3e} (bound {2 * U * gain * gs:.3e})")
        assert d_g <= 2 * U * gain * gs
    # the same launches as the autograd path on the half batch: bit for bit
    got = [g.clone() for _, g in s16.param_grads]
    a_pred, a_loss, a_score, a_grads, _ = _autograd(model, d16, "resident")
    assert torch.equal(a_pred, s16.pred) and torch.equal(a_loss, s16.loss) and torch.equal(a_score, s16.score)
    names = {id(p): n for n, p in model.named_parameters()}
    for (p, _), g in zip(s16.param_grads, got):
        assert torch.equal(a_grads[names[id(p)]], g), names[id(p)]


def test_captured_step_replays_and_follows_the_parameters():
    from graph_hscn.replay import CapturedStep, StaticHeteroBatch
    from graph_hscn.step import ResidentTrainStep
    C = 10
    hb = _batch(6, C, 9)
    static = StaticHeteroBatch([hb], DEV)
    assert static.class_index and static.batch["local"].y.dtype == torch.int64
    static.load(hb.to(DEV))
    model = _model(C)
    cs = CapturedStep(model, static, "cross_entropy")
    assert cs.step.class_index
    losses = []
    for _ in range(3):
        losses.append(cs.replay().clone())
    torch.cuda.synchronize()
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[1], losses[2])
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(DEV))
    got = cs.replay().clone()
    got_grads, got_score = cs.step.grads.clone(), cs.score.clone()
    fresh = ResidentTrainStep(model, static.batch, "cross_entropy")
    fresh.run()
    torch.cuda.synchronize()
    assert not torch.equal(got, losses[0])
    assert torch.equal(got, fresh.loss) and torch.equal(got_score, fresh.score)
    assert torch.equal(got_grads[:fresh.P], fresh.grads[:fresh.P])


def _eval_epoch(model, graphs, B, metric_fn):
    from graph_hscn.data import DataLoader
    from graph_hscn.train import train as T
    keep, training = model.engine, model.training
    model.engine = "resident"
    try:
        return T.eval_epoch(0, None, DataLoader(graphs, batch_size=B), model, "cross_entropy", metric_fn, "Validation")
    finally:
        model.engine = keep
        model.train(training)


@pytest.mark.parametrize("metric", ["accuracy", "f1_macro"])
def test_fit_resident_and_the_device_evaluator(metric):
    from graph_hscn import metrics as M
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    C, B = 3, 4
    hs = _graphs(32, C, seed=12)
    train, val, test = hs[:12], hs[12:22], hs[22:32]            # evaluation splits: 2 gathered batches + a tail of 2
    metric_fn = M.eval_accuracy if metric == "accuracy" else M.eval_f1_macro
    tc = TrainingConfig("hscn", "cross_entropy", metric, epochs=2, eval_period=1, patience=50)
    cfg = OptimConfig("adamW", lr=0.01)
    model = _model(C)
    before = [p.detach().clone() for p in model.parameters()]
    evals = []
    hist = fit_resident(None, cfg, tc, train, None, model, batch_size=B, eval_graphs=(val, test), metric=metric,
                        eval_history=evals)
    assert len(hist) == 2 and all(np.isfinite(l) and 0.0 <= p <= 1.0 for l, p in hist)
    assert len(evals) == 4 and all(np.isfinite(e[2]) and 0.0 <= e[3] <= 1.0 for e in evals)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    # the same loop with the torch definition as metric_fn: the same history
    model2 = _model(C)
    hist2 = fit_resident(None, cfg, tc, train, None, model2, batch_size=B, metric_fn=metric_fn)
    assert [h[0] for h in hist2] == [h[0] for h in hist]
    assert all(abs(a[1] - b[1]) <= 1e-12 for a, b in zip(hist, hist2))
    # the evaluator against eval_epoch on the same split and weights
    ev = DeviceEvaluator(val, model, "cross_entropy", B, metric)
    assert (ev.steps, ev.tail, ev.num_batches) == (2, 2, 3) and ev.class_index and ev.C == C
    loss, perf = ev.evaluate()
    run = ev.run()
    assert run.targets.dtype == torch.int64 and torch.equal(run.targets.cpu(), torch.cat([h["local"].y for h in val]))
    want_loss, want_perf = _eval_epoch(model, val, B, metric_fn)
    assert loss == want_loss                                    # tests/test_gpu_eval_resident.py: the same launches
    if metric == "accuracy":
        assert perf == want_perf
    else:
        assert abs(perf - want_perf) <= 1e-12
    assert (loss, perf) == ev.evaluate()
    with pytest.raises(ValueError, match="does not fit"):
        DeviceEvaluator(val, model, "cross_entropy", B, "ap")
