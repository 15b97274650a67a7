"""Gradient accumulation and norm clipping in the captured training loop (reference train/train.py:89-95:
``batch_accumulation`` and ``clip_grad_norm``): the clip inside the one-launch optimizer and on its own against
torch's ``clip_grad_norm_``, the accumulating gradient fold bit for bit, and ``fit_resident`` with both settings
against ``train.train_epoch`` replayed over the same batch order."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- the clip against torch on synthetic flat buffers -------------------------------------------------------------

def _ulps(a, b):
    """|a - b| in units of b's spacing (float32)."""
    up = torch.nextafter(b, torch.full_like(b, float("inf")))
    return ((a.double() - b.double()).abs() / (up.double() - b.double()).abs()).max().item()


def _flat(P, scale, seed, sizes=None):
    g = torch.Generator().manual_seed(seed)
    flat = (torch.randn(P + 1, generator=g) * scale).to(DEV)      # (+1: the loss column the steps carry)
    sizes = sizes or [P // 3, P // 3, P - 2 * (P // 3)]
    params, off = [], 0
    for n in sizes:
        params.append(torch.randn(n, generator=g).to(DEV))
        off += n
    return flat, params


def _torch_clip(grads, sizes, max_norm=1.0):
    ps = []
    off = 0
    for n in sizes:
        p = torch.zeros(n, device=DEV, requires_grad=True)
        p.grad = grads[off:off + n].clone()
        ps.append(p)
        off += n
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return torch.cat([p.grad for p in ps]), norm


@pytest.mark.parametrize("P", [1146, 5000, 9001])
@pytest.mark.parametrize("mode", ["standalone", "flat_adam", "flat_adam_captured"])
def test_clip_matches_torch(P, mode):
    from graph_hscn.optim import FlatAdam, clip_grad_norm_flat
    for scale, engaged in ((1.0, True), (1e-3, False)):
        flat, params = _flat(P, scale, seed=P)
        sizes = [p.numel() for p in params]
        before = flat.clone()
        referee = float(before[:P].double().norm())
        assert (referee > 1.0) == engaged
        want, want_norm = _torch_clip(before[:P], sizes)
        if mode == "standalone":
            norm = torch.zeros(1, device=DEV)
            clip_grad_norm_flat(flat[:P], 1.0, norm)
        else:
            off, pg = 0, []
            for p in params:
                pg.append((p, flat[off:off + p.numel()]))
                off += p.numel()
            p0 = [p.clone() for p in params]
            opt = FlatAdam(pg, flat[:P], lr=1e-2, weight_decay=0.01, decoupled=True, max_norm=1.0)
            if mode == "flat_adam_captured":
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    opt.step()
                g.replay()
            else:
                opt.step()
            norm = opt.last_norm
            torch.cuda.synchronize()
            assert float(opt.step_count) == 1.0
            # the update took the clipped gradient: a plain step on the buffer the clip left is the same step
            q = [p.clone() for p in p0]
            off, qg = 0, []
            g2 = flat[:P].clone()
            for p in q:
                qg.append((p, g2[off:off + p.numel()]))
                off += p.numel()
            FlatAdam(qg, g2, lr=1e-2, weight_decay=0.01, decoupled=True).step()
            torch.cuda.synchronize()
            for a, b in zip(params, q):
                assert torch.equal(a, b)
        torch.cuda.synchronize()
        got = flat[:P]
        assert abs(float(norm) - referee) <= 1e-6 * referee
        assert abs(float(norm) - float(want_norm)) <= 1e-6 * referee
        assert torch.equal(flat[P], before[P])                       # the loss column is not a gradient
        if engaged:
            assert _ulps(got, want) <= 2.0
            assert float(got.double().norm()) < 1.0 + 1e-5
        else:
            assert torch.equal(got.view(torch.int32), before[:P].view(torch.int32))   # bitwise unchanged


def test_flat_adam_zero_after_update_and_nonfinite_norm():
    from graph_hscn.optim import FlatAdam, clip_grad_norm_flat
    flat, params = _flat(1146, 1.0, seed=1)
    off, pg = 0, []
    for p in params:
        pg.append((p, flat[off:off + p.numel()]))
        off += p.numel()
    opt = FlatAdam(pg, flat[:1146], lr=1e-2, zero_grads=True)
    opt.step()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(flat[:1146])) == 0
    # a non-finite gradient propagates as in torch (no special case): NaN / inf norm -> NaN / zero scale
    for bad in (float("nan"), float("inf")):
        g = torch.randn(1146, device=DEV)
        g[7] = bad
        want, want_norm = _torch_clip(g, [1146])
        norm = torch.zeros(1, device=DEV)
        clip_grad_norm_flat(g, 1.0, norm)
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(g), torch.isnan(want))
        assert float(norm) == float(want_norm) or (np.isnan(float(norm)) and np.isnan(float(want_norm)))


def test_clip_norm_is_reproducible():
    from graph_hscn.optim import clip_grad_norm_flat
    base = torch.randn(9001, device=DEV) * 3
    norms = []
    for _ in range(3):
        g = base.clone()
        n = torch.zeros(1, device=DEV)
        clip_grad_norm_flat(g, 1.0, n)
        torch.cuda.synchronize()
        norms.append((n.clone(), g))
    for n, g in norms[1:]:
        assert torch.equal(n, norms[0][0]) and torch.equal(g, norms[0][1])


# ---- the accumulating fold on the captured step -------------------------------------------------------------------

def _batches(B, K, C, seeds):
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    rng = np.random.default_rng(0)
    out = []
    for seed in seeds:
        graphs = make_dataset("peptides_func", B, seed=seed)
        for g in graphs:
            g.y = torch.from_numpy((rng.random((1, C)) < 0.3).astype(np.float32))
        out.append(HeteroBatch.from_data_list(
            [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]))
    return out


@pytest.mark.parametrize("form", ["one_launch", "pair", "pair_plain", "one_launch_f16", "pair_f16"])
def test_accumulating_step_sums_micro_batch_gradients_exactly(form):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.replay import CapturedStep, StaticHeteroBatch
    batches = _batches(6, 16, 10, (1, 2, 3))
    torch.manual_seed(0)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(DEV)
    model.engine = "resident"
    if form == "pair_plain":
        model.overlap_virtual = False           # the launch pair without the virtual workgroups: hscn_resident_bwd
    fdt = torch.float16 if form.endswith("f16") else torch.float32
    one_launch = True if form.startswith("one_launch") else False
    static = StaticHeteroBatch(batches, DEV, feature_dtype=fdt)
    plain = CapturedStep(model, static, "cross_entropy", one_launch=one_launch)
    P = plain.step.P
    g, losses = [], []
    for hb in batches:
        static.load(hb)
        plain.replay()
        torch.cuda.synchronize()
        g.append(plain.step.grads[:P].clone())
        losses.append(plain.loss.clone())
    acc = CapturedStep(model, static, "cross_entropy", one_launch=one_launch, accumulate=True)
    assert acc.step.one_launch == plain.step.one_launch == one_launch
    assert int(torch.count_nonzero(acc.step.grads[:P])) == 0           # the warm-up's gradients are gone
    want = torch.zeros_like(g[0])
    for i, hb in enumerate(batches):
        static.load(hb)
        acc.replay(step_optimizer=False)
        torch.cuda.synchronize()
        want = want + g[i]
        assert torch.equal(acc.step.grads[:P], want), i                 # ((g1 + g2) + g3), bit for bit
        assert torch.equal(acc.loss, losses[i]), i                      # the loss of THIS micro-batch
    assert torch.equal(want, (g[0] + g[1]) + g[2])


# ---- fit_resident with both settings ------------------------------------------------------------------------------

def _data(n, seed, feat_scale):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("peptides_func", n, seed=seed)
    rng = np.random.default_rng(seed)
    hs = [hetero_from_clusters(g, rng.integers(0, 8, g.num_nodes), 8) for g in graphs]
    for h in hs:                               # larger inputs: gradient norms well above 1, the clip engages
        h["local"].x = h["local"].x.float() * feat_scale
        h["virtual"].x = h["virtual"].x.float() * feat_scale
    return hs


def _model():
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(0)
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(DEV)


def _record_flat_adams(monkeypatch):
    from graph_hscn.optim import FlatAdam
    made = []
    orig = FlatAdam.from_config.__func__

    def from_config(cls, *a, **kw):
        opt = orig(cls, *a, **kw)
        made.append(opt)
        return opt

    monkeypatch.setattr(FlatAdam, "from_config", classmethod(from_config))
    return made


def test_fit_resident_accumulates_and_clips_like_train_epoch(monkeypatch):
    from graph_hscn.config.config import OPTIM_DICT, OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.train import train as T
    from graph_hscn.train.train_resident import fit_resident, optimizer_steps_at
    hs = _data(54, 11, 5.0)
    G, B, k, epochs = 44, 8, 3, 3                  # 5 captured batches + a 4-graph eager tail: steps at it 2 and 5
    train, loaders = hs[:G], [DataLoader(hs[G:49], batch_size=5), DataLoader(hs[49:], batch_size=5)]
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=epochs, eval_period=epochs, patience=50)
    cfg = OptimConfig("adamW", batch_accumulation=k, clip_grad_norm=True, lr=0.01)
    made = _record_flat_adams(monkeypatch)
    model = _model()
    orders = []
    hist = fit_resident(None, cfg, tc, train, loaders, model, batch_size=B, epoch_orders=orders)
    assert len(hist) == epochs and len(orders) == epochs and len(made) == 1
    nb = G // B + 1
    assert float(made[0].step_count) == epochs * sum(optimizer_steps_at(i, nb, k) for i in range(nb))
    for o in orders:
        assert o.device.type == "cpu" and sorted(o.tolist()) == list(range(G))
    # the reference-shaped loop over the same batch order, torch's AdamW and clip_grad_norm_
    norms = []
    clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(params, max_norm, *a, **kw):
        n = clip(params, max_norm, *a, **kw)
        norms.append(float(n))
        return n

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", recording_clip)
    ref = _model()
    opt = OPTIM_DICT["adamW"](ref.parameters(), lr=0.01, weight_decay=cfg.weight_decay)
    for e, o in enumerate(orders):
        loader = DataLoader([train[j] for j in o.tolist()], batch_size=B)
        T.train_epoch(e, None, loader, ref, opt, "cross_entropy", None, k, True)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", clip)
    assert len(norms) == float(made[0].step_count)
    assert max(norms) > 1.0                                             # the clip engaged
    assert float(made[0].last_norm) == pytest.approx(norms[-1], rel=1e-2)

    def dist(a, b):
        return max(float((p - q).detach().abs().max()) / max(1.0, float(q.detach().abs().max()))
                   for p, q in zip(a.parameters(), b.parameters()))

    assert dist(model, ref) <= 2e-4
    # torch's capturable fused AdamW in the graph (the clip as its own launch) takes the same trajectory
    model3 = _model()
    fit_resident(None, cfg, tc, train, loaders, model3, batch_size=B, flat_optimizer=False)
    assert dist(model3, ref) <= 2e-4
    # and without the clip the run ends elsewhere
    model2 = _model()
    fit_resident(None, OptimConfig("adamW", batch_accumulation=k, lr=0.01), tc, train, loaders, model2, batch_size=B)
    assert dist(model2, model) > 2e-4


def _reducer_of_one_equals_no_reducer(cfg, num_train, epochs, port, flat_optimizer=True):
    """fit_resident with a world-of-one RCCL reducer against the same run without a reducer: parameters bit for bit."""
    import torch.distributed as dist
    from graph_hscn.config.config import TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.distributed import FlatGradReducer
    from graph_hscn.train.train_resident import fit_resident
    hs = _data(num_train + 10, 5, 1.0)
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=epochs, eval_period=epochs, patience=50)
    loaders = [DataLoader(hs[num_train:num_train + 5], batch_size=5), DataLoader(hs[num_train + 5:], batch_size=5)]

    def run(reducer_factory):
        m = _model()
        fit_resident(None, cfg, tc, hs[:num_train], loaders, m, batch_size=8,
                     reducer=reducer_factory(m) if reducer_factory else None, flat_optimizer=flat_optimizer)
        return [p.detach().clone() for p in m.parameters()]

    want = run(None)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        got = run(lambda m: FlatGradReducer(m, single_rank_collective=True))
    finally:
        dist.destroy_process_group()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_fit_resident_accumulation_with_the_rccl_reducer_single_rank():
    """k = 3 with the all-reduce captured in the boundary graph only: a world of one gives the parameters of the
    single-process loop, bit for bit."""
    from graph_hscn.config.config import OptimConfig
    _reducer_of_one_equals_no_reducer(OptimConfig("adamW", batch_accumulation=3, clip_grad_norm=True, lr=0.01),
                                      num_train=30, epochs=3, port=29583)


@pytest.mark.parametrize("flat_optimizer", [True, False])
def test_fit_resident_without_accumulation_or_clip_with_the_rccl_reducer_single_rank(flat_optimizer):
    """k = 1, no clip: 20 graphs in batches of 8 are two captured batches and a 4-graph eager tail, whose gradients
    are reduced in the flat buffer like the captured ones.  Bit for bit the run without a reducer, with the one-launch
    AdamW and with torch's."""
    from graph_hscn.config.config import OptimConfig
    _reducer_of_one_equals_no_reducer(OptimConfig("adamW", batch_accumulation=1, clip_grad_norm=False, lr=0.01),
                                      num_train=20, epochs=2, port=29584 + int(flat_optimizer),
                                      flat_optimizer=flat_optimizer)


def test_fit_resident_non_capturable_optimizer_accumulates_and_clips():
    """Adagrad (no capturable step): the micro-batch graph, then the clip as its own launch and the eager step."""
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.train.train_resident import fit_resident
    hs = _data(60, 3, 1.0)
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=6, eval_period=6, patience=50)
    loaders = [DataLoader(hs[50:55], batch_size=5), DataLoader(hs[55:], batch_size=5)]
    model = _model()
    hist = fit_resident(None, OptimConfig("adagrad", batch_accumulation=2, clip_grad_norm=True, lr=0.05), tc, hs[:50],
                        loaders, model, batch_size=8)
    assert all(np.isfinite(l) for l, _ in hist)
    assert hist[-1][0] < hist[0][0]
