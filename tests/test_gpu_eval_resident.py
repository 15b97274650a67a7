"""``train.eval_resident.DeviceEvaluator`` against ``train.eval_epoch`` over an in-order host loader of the same
graphs, and ``fit_resident`` with the device evaluation path against the loader path.

Both sides run one chain per batch -- gather or host collation, the model's forward-only resident launch,
``hscn_criterion_fwd`` -- so scores, targets, per-batch losses and their float32 mean are required to be equal bit
for bit; that the gathered batch IS the host-collated one is asserted first so that a failure localises.  The metric
is held to the a-priori bounds of tests/test_gpu_metrics.py (AP: 8 G 2^-53 absolute; MAE: (G C + 2) 2^-53 relative)
against the torch restatement on the same device tensors."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53
LL, VV, LV = ("local", "to", "local"), ("virtual", "to", "virtual"), ("local", "to", "virtual")


def _hetero(name, G, K, seed):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    rng = np.random.default_rng(seed)
    return [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in make_dataset(name, G, seed=seed)]


def _hscn(C, seed=0):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(seed)
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, C, 3).to(DEV)


def _mpnn(seed=0):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(seed)
    return MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 10, 3, 0.1).to(DEV)


def _setup(which, G):
    """(graphs, model, loss_fn, metric name, metric_fn)"""
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.metrics import eval_ap, eval_mae
    if which == "hscn_bce":
        return _hetero("peptides_func", G, 8, seed=21), _hscn(10), "cross_entropy", "ap", eval_ap
    if which == "hscn_l1":
        return _hetero("peptides_struct", G, 8, seed=22), _hscn(11), "l1", "mae", eval_mae
    return make_dataset("peptides_func", G, seed=23), _mpnn(), "cross_entropy", "ap", eval_ap


def _same_hetero(static_hb, host):
    for nt in ("local", "virtual"):
        n = host[nt].num_nodes
        assert torch.equal(static_hb[nt].x[:n].cpu(), host[nt].x.float())
        assert torch.equal(static_hb[nt].batch[:n].cpu(), host[nt].batch)
        assert torch.equal(static_hb[nt].ptr.cpu(), host[nt].ptr) and torch.equal(static_hb[nt].ptr32.cpu(), host[nt].ptr32)
    assert torch.equal(static_hb["local"].y.cpu(), host["local"].y.float())
    for et in (LL, VV, LV):
        e = host[et].edge_index.size(1)
        assert torch.equal(static_hb[et].edge_index[:, :e].cpu(), host[et].edge_index)
        assert torch.equal(static_hb[et].ptr32.cpu(), host[et].ptr32)


def _same_graph(static_b, host):
    n, e = host.x.size(0), host.edge_index.size(1)
    assert torch.equal(static_b.x[:n].cpu(), host.x.float()) and torch.equal(static_b.batch[:n].cpu(), host.batch)
    assert torch.equal(static_b.edge_index[:, :e].cpu(), host.edge_index)
    assert torch.equal(static_b.ptr.cpu(), host.ptr) and torch.equal(static_b.ptr32.cpu(), host.ptr32)
    assert torch.equal(static_b.eptr32.cpu(), host.eptr32) and torch.equal(static_b.y.cpu(), host.y.float())


def _metric_close(metric, got, want, G, C):
    if metric == "ap":
        print(f"AP |delta| {abs(got - want):.3e}, bound {8 * G * U:.3e}")
        return abs(got - want) <= 8 * G * U
    print(f"MAE relative error {abs(got - want) / want:.3e}, bound {(G * C + 2) * U:.3e}")
    return abs(got - want) / want <= (G * C + 2) * U


def _eval_epoch_recorded(monkeypatch, loader, model, loss_fn, metric_fn):
    """train.eval_epoch with its per-batch losses and the tensors its metric saw."""
    from graph_hscn.train import train as T
    real, seen = T.criterion, {"losses": []}

    def criterion(*a):
        loss, score = real(*a)
        seen["losses"].append(loss.clone())
        return loss, score

    def metric(t, s):
        seen["targets"], seen["scores"] = t.clone(), s.clone()
        return metric_fn(t, s)

    monkeypatch.setattr(T, "criterion", criterion)
    seen["loss"], seen["perf"] = T.eval_epoch(0, None, loader, model, loss_fn, metric, "Validation")
    monkeypatch.setattr(T, "criterion", real)
    return seen


@pytest.mark.parametrize("which", ["hscn_bce", "hscn_l1", "mpnn_bce"])
def test_device_evaluator_equals_eval_epoch(which, monkeypatch):
    from graph_hscn.data import DataLoader, collate
    from graph_hscn.train.eval_resident import DeviceEvaluator
    G, B = 75, 16                                    # 4 gathered batches + an 11-graph tail
    graphs, model, loss_fn, metric, metric_fn = _setup(which, G)
    model.engine = "resident"
    model.train()
    ev = DeviceEvaluator(graphs, model, loss_fn, B, metric)
    assert (ev.steps, ev.tail, ev.num_batches) == (4, 11, 5)
    for i in range(ev.steps):                        # the gathered batch is the host-collated one, bit for bit
        got = ev.ds.gather(ev.ids[i])
        (_same_graph if which == "mpnn_bce" else _same_hetero)(got, collate(graphs[i * B:(i + 1) * B]))
    ev.ds.check()
    want = _eval_epoch_recorded(monkeypatch, DataLoader(graphs, batch_size=B), model, loss_fn, metric_fn)
    assert model.last_engine == "resident" and len(want["losses"]) == 5
    model.train()
    run = ev.run()
    assert model.training and model.engine == "resident" and model.last_engine == "resident"
    C = run.scores.size(1)
    assert torch.equal(run.targets, want["targets"].float()) and torch.equal(run.scores, want["scores"])
    assert torch.equal(run.loss_log, torch.stack(want["losses"]))
    assert float(run.loss) == want["loss"]
    got_metric = float(run.metric.result[0])
    assert _metric_close(metric, got_metric, want["perf"], G, C)
    loss, perf = ev.evaluate()                       # (a second evaluation into the same buffers: the same bits)
    assert loss == want["loss"] and perf == got_metric
    model.eval()
    ev.run()
    assert not model.training
    # without a metric: the loss alone, NaN for the metric, as eval_epoch answers without a metric_fn
    loss, perf = DeviceEvaluator(graphs, model, loss_fn, B).evaluate()
    assert loss == want["loss"] and perf != perf


def test_a_split_smaller_than_one_batch_and_one_without_a_tail(monkeypatch):
    from graph_hscn.data import DataLoader
    from graph_hscn.metrics import eval_ap
    from graph_hscn.train.eval_resident import DeviceEvaluator
    graphs = _hetero("peptides_func", 32, 8, seed=5)
    model = _hscn(10)
    model.engine = "resident"
    for part, B in ((graphs[:7], 16), (graphs, 16)):
        want = _eval_epoch_recorded(monkeypatch, DataLoader(part, batch_size=B), model, "cross_entropy", eval_ap)
        ev = DeviceEvaluator(part, model, "cross_entropy", B, "ap")
        loss, perf = ev.evaluate()
        assert loss == want["loss"] and abs(perf - want["perf"]) <= 8 * len(part) * U
        assert torch.equal(ev.scores, want["scores"])


def test_run_reads_nothing_back_and_evaluate_reads_once():
    from graph_hscn.train.eval_resident import DeviceEvaluator
    graphs, model, loss_fn, metric, _ = _setup("hscn_bce", 40)
    ev = DeviceEvaluator(graphs, model, loss_fn, 16, metric)
    ev.evaluate()                                    # warm-up: code objects loaded, buffers cached
    one = torch.ones(1, device=DEV)
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            one.item()
            implemented = False
        except RuntimeError:
            implemented = True
        if implemented:
            ev.run()                                 # raises on any synchronising call
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                ev.evaluate()
            syncs = [w for w in caught if "synchroniz" in str(w.message).lower()]
            assert len(syncs) == 1, [str(w.message) for w in caught]
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not implemented:
        print("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build: the read-back "
              "assertions were not made")


def test_fit_resident_device_evaluation_equals_the_loader_path():
    """The same seed, the same graphs, evaluation every epoch, early stopping after the third epoch (min_delta is
    larger than any loss, so only the first evaluation counts as an improvement; patience 2)."""
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.metrics import eval_ap
    from graph_hscn.train.train_resident import fit_resident
    hs = _hetero("peptides_func", 78, 8, seed=9)
    train, val, test = hs[:44], hs[44:65], hs[65:]   # B = 8: 5 steps + a 4-graph tail; 21 = 2 * 8 + 5; 13 = 8 + 5
    B = 8
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=8, eval_period=1, min_delta=10.0, patience=2)
    cfg = OptimConfig("adamW", lr=0.01)
    m1, m2 = _hscn(10, seed=4), _hscn(10, seed=4)
    h1, h2 = [], []
    hist1 = fit_resident(None, cfg, tc, train, None, m1, batch_size=B, eval_graphs=(val, test), metric="ap",
                         eval_history=h1)
    hist2 = fit_resident(None, cfg, tc, train, [DataLoader(val, batch_size=B), DataLoader(test, batch_size=B)], m2,
                         batch_size=B, metric_fn=eval_ap, eval_history=h2)
    assert len(hist1) == len(hist2) == 3             # stopped early, at the same epoch
    assert [l for l, _ in hist1] == [l for l, _ in hist2]
    for (_, a), (_, b) in zip(hist1, hist2):
        assert abs(a - b) <= 8 * len(train) * U
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p, q)
    assert [(e, s) for e, s, _, _ in h1] == [(e, s) for e, s, _, _ in h2] == \
        [(0, "Validation"), (0, "Test"), (1, "Validation"), (1, "Test"), (2, "Validation")]   # (the stop precedes Test)
    for (_, split, la, pa), (_, _, lb, pb) in zip(h1, h2):
        assert la == lb, (split, la, lb)
        assert abs(pa - pb) <= 8 * len(val if split == "Validation" else test) * U
    # the HIP metric over host loaders (metric= without eval_graphs) takes the same path through eval_epoch
    m3, h3 = _hscn(10, seed=4), []
    fit_resident(None, cfg, tc, train, [DataLoader(val, batch_size=B), DataLoader(test, batch_size=B)], m3,
                 batch_size=B, metric="ap", eval_history=h3)
    assert [(e, s, l) for e, s, l, _ in h3] == [(e, s, l) for e, s, l, _ in h1]
    assert [p for *_, p in h3] == [p for *_, p in h1]
