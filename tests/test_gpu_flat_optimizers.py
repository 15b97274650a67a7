"""The one-launch optimizers at the shapes where their kernel branches (csrc/optim.hip): ``FlatAdam`` (Adam / AdamW) and
``FlatAdagrad`` against torch's CPU optimizers in float32 and float64 on the same synthetic gradients, schedules
evaluated inside the launch against ``LRSchedule.factor`` / ``LambdaLR``, capture and replay, and ``fit_resident`` with
Adagrad and with a scheduled AdamW.

The bar for parameters is the referee of tests/test_gpu_mpnn_resident.py, per parameter tensor and after every step:

    |HIP - f64|  <=  2 |torch_f32 - f64| + 8 ulp(scale),      ulp(scale) = 2^-23 max|f64|

(the kernel and torch's float32 are two roundings of one function: no tolerance is invented)."""
import functools
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPS = 12
MAX_NORM = 1.0

# name -> (torch class, its keywords, flat class name, its keywords)
VARIANTS = {
    "adam": (torch.optim.Adam, dict(lr=1e-2), "FlatAdam", dict(lr=1e-2, decoupled=False)),
    "adamW": (torch.optim.AdamW, dict(lr=1e-2), "FlatAdam", dict(lr=1e-2, decoupled=True)),
    "adagrad": (torch.optim.Adagrad, dict(lr=5e-2), "FlatAdagrad", dict(lr=5e-2)),
    "adagrad_decay": (torch.optim.Adagrad, dict(lr=5e-2, lr_decay=0.1), "FlatAdagrad", dict(lr=5e-2, lr_decay=0.1)),
    "adagrad_iav": (torch.optim.Adagrad, dict(lr=5e-2, initial_accumulator_value=0.1), "FlatAdagrad",
                    dict(lr=5e-2, initial_accumulator_value=0.1)),
    "adagrad_decay_iav": (torch.optim.Adagrad, dict(lr=5e-2, lr_decay=0.1, initial_accumulator_value=0.1),
                          "FlatAdagrad", dict(lr=5e-2, lr_decay=0.1, initial_accumulator_value=0.1)),
}
# 4 x 1024 elements are held in registers, the rest goes through the tail loop
SIZES = [1, 1023, 1024, 4096, 4097, 5000]
CLIPS = ["off", "below", "above"]


@functools.lru_cache(maxsize=None)
def _inputs(P, clip):
    """Initial parameters [P] and the STEPS gradients [STEPS, P] (float32, host): torch.randn with a fixed seed, scaled
    per step -- to a 2-norm below / above MAX_NORM where the clip is to stay idle / to engage."""
    gen = torch.Generator().manual_seed(1000 + P)
    p0 = torch.randn(P, generator=gen)
    g = torch.randn(STEPS, P, generator=gen)
    for t in range(STEPS):
        if clip == "off":
            g[t] *= 0.5 + 0.1 * t
        else:
            target = (0.2 + 0.05 * t) if clip == "below" else (1.5 + 0.3 * t)
            g[t] *= target / float(g[t].double().norm())
    return p0, g


@functools.lru_cache(maxsize=None)
def _reference(variant, P, wd, clip, schedule_key=None):
    """Parameters after every step from torch's CPU optimizer in float32 and float64: ``(p32 [STEPS, P], p64)``.
    Computed once per setting and shared (the segment tables and the zeroing do not change the trajectory)."""
    cls, kw = VARIANTS[variant][:2]
    p0, g = _inputs(P, clip)
    out = []
    for dt in (torch.float32, torch.float64):
        p = torch.nn.Parameter(p0.to(dt).clone())
        opt = cls([p], weight_decay=wd, **kw)
        sched = None
        if schedule_key is not None:
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=_schedule(schedule_key).as_lambda())
        traj = torch.empty(STEPS, P, dtype=dt)
        for t in range(STEPS):
            p.grad = g[t].to(dt).clone()
            if clip != "off":
                torch.nn.utils.clip_grad_norm_([p], MAX_NORM)
            opt.step()
            if sched is not None:
                sched.step()
            traj[t] = p.detach()
        out.append(traj)
    return tuple(out)


def _schedule(key):
    from graph_hscn.optim import LRSchedule
    kind, warmup, total, period, gamma, min_factor = key
    return LRSchedule(kind, warmup_steps=warmup, total_steps=total, period=period, gamma=gamma, min_factor=min_factor)


def _segments(P, nseg):
    """``nseg`` uneven positive sizes that sum to P."""
    if nseg == 1:
        return [P]
    cuts = sorted(random.Random(P).sample(range(1, P), nseg - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [P])]


class _Flat:
    """A flat gradient buffer (+ the loss column the steps carry) and parameter tensors that lie in REVERSED segment
    order inside one backing buffer: a wrong table lookup lands in another tensor, one copy reads them all back."""

    def __init__(self, p0, sizes):
        P = sum(sizes)
        self.P, self.sizes = P, sizes
        self.grads = torch.zeros(P + 1, device=DEV)
        self.grads[P] = 123.0
        self.backing = torch.zeros(P, device=DEV)
        self.params, self.views, self.where = [], [], []
        off, end = 0, P
        for n in sizes:
            end -= n
            q = self.backing[end:end + n]
            q.copy_(p0[off:off + n])
            self.params.append(q)
            self.views.append((q, self.grads[off:off + n]))
            self.where.append((off, end, n))
            off += n

    def read(self):
        """The parameters in flat order, on the host."""
        b = self.backing.cpu()
        return torch.cat([b[end:end + n] for _, end, n in self.where])


def _build(variant, flat, **kw):
    from graph_hscn import optim
    name, fkw = VARIANTS[variant][2:]
    return getattr(optim, name)(flat.views, flat.grads[:flat.P], **dict(fkw, **kw))


def _refereed(hip, p32, p64, sizes, what):
    lengths = torch.tensor(sizes)
    seg_max = lambda x: torch.segment_reduce(x, "max", lengths=lengths)
    h, a, r = hip.double(), p32.double(), p64.double()
    e_hip, e_32, ulp = seg_max((h - r).abs()), seg_max((a - r).abs()), 2.0 ** -23 * seg_max(r.abs())
    bad = torch.nonzero(~(e_hip <= 2.0 * e_32 + 8.0 * ulp)).flatten().tolist()
    if bad:
        k = bad[0]
        print(f"[f64 referee] {what}: segments {bad[:8]}; segment {k} (size {sizes[k]}): |HIP-f64|={float(e_hip[k]):.3e} "
              f"|torch32-f64|={float(e_32[k]):.3e} ulp(scale)={float(ulp[k]):.3e}")
    return not bad


def _clip_coef(norm: torch.Tensor) -> torch.Tensor:
    """torch's clip_grad_norm_ from the norm on, in float32 (what the kernel applies)."""
    one = torch.ones((), dtype=torch.float32)
    return torch.clamp((one / (norm.cpu() + torch.tensor(1e-6, dtype=torch.float32))) * MAX_NORM, max=1.0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_against_reference(variant, P, nseg, wd, clip, zero, schedule_key=None):
    p0, g = _inputs(P, clip)
    p32, p64 = _reference(variant, P, wd, clip, schedule_key)
    sizes = _segments(P, nseg)
    flat = _Flat(p0, sizes)
    kw = dict(weight_decay=wd, max_norm=MAX_NORM if clip != "off" else None, zero_grads=zero)
    if schedule_key is not None:
        kw["schedule"] = _schedule(schedule_key)
    opt = _build(variant, flat, **kw)
    g_dev = g.to(DEV)
    tag = f"{variant} P={P} nseg={nseg} wd={wd} clip={clip} zero={zero} sched={schedule_key}"
    for t in range(STEPS):
        flat.grads[:P].copy_(g_dev[t])
        opt.step()
        got = flat.read()                                  # (synchronizes)
        assert float(opt.step_count) == t + 1
        assert _refereed(got, p32[t], p64[t], sizes, f"{tag} step {t}"), (tag, t)
        left = flat.grads.cpu()
        assert float(left[P]) == 123.0                     # the loss column is not a gradient
        if clip != "off":
            norm64 = float(g[t].double().norm())
            assert (norm64 > MAX_NORM) == (clip == "above")
            assert abs(float(opt.last_norm) - norm64) <= 1e-6 * norm64
        if zero:
            assert int(torch.count_nonzero(_bits(left[:P]))) == 0, (tag, t)
        elif clip != "off":
            want = g[t] * _clip_coef(opt.last_norm)
            assert torch.equal(_bits(left[:P]), _bits(want)), (tag, t)
            if clip == "below":
                assert torch.equal(_bits(want), _bits(g[t]))
        else:
            assert torch.equal(_bits(left[:P]), _bits(g[t])), (tag, t)
    opt.check()


@pytest.mark.parametrize("nseg", [1, 64])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_flat_optimizer_matches_torch_within_the_f64_referee(variant, P, nseg):
    nseg = min(nseg, P)                                    # (P = 1 has one segment either way)
    for wd in (0.0, 5e-4):
        for clip in CLIPS:
            for zero in (False, True):
                _run_against_reference(variant, P, nseg, wd, clip, zero)


# ---- schedules inside the launch ------------------------------------------------------------------------------------

SCHEDULES = {
    "cosine": ("cosine_with_warmup", 3, 8, 1, 1.0, 0.05),
    "linear": ("linear_with_warmup", 3, 8, 1, 1.0, 0.0),
    "step": ("step", 0, 8, 4, 0.7, 0.0),
    "step_every": ("step", 0, 8, 1, 0.7, 0.0),
}


def _within_ulps(a, b, n=4):
    return abs(a - b) <= n * math.ulp(b)


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("variant", ["adamW", "adam", "adagrad_decay"])
def test_schedule_in_the_launch_matches_the_host_formula_and_lambda_lr(variant, name):
    key = SCHEDULES[name]
    sch = _schedule(key)
    P, sizes = 5000, _segments(5000, 3)
    p0, g = _inputs(P, "above")
    flat = _Flat(p0, sizes)
    opt = _build(variant, flat, weight_decay=5e-4, max_norm=MAX_NORM, schedule=sch)
    base = opt.lr
    assert opt.schedule.base_lr == base and sch.base_lr is None        # the caller's record is left alone
    assert opt.last_lr.dim() == 0 and opt.last_lr.dtype == torch.float64
    assert float(opt.last_lr) == base * sch.factor(0)
    with pytest.raises(RuntimeError):
        opt.set_lr(0.5)
    if variant != "adagrad_decay":
        with pytest.raises(RuntimeError):
            opt.c
    g_dev = g.to(DEV)
    seen = []
    for s in range(STEPS):
        flat.grads[:P].copy_(g_dev[s])
        opt.step()
        lr = float(opt.last_lr)
        want = base * sch.factor(s)
        print(f"{variant} {name} step {s}: device lr {lr!r} host {want!r}")
        assert _within_ulps(lr, want), (s, lr, want)
        if key[0] != "cosine_with_warmup":
            assert lr == want, (s, lr, want)               # the rational kinds and the running product are exact
        seen.append(lr)
    assert seen[8:] == [seen[8]] * 4 if key[0] != "step" else seen[8] < seen[7]     # clamped behind total_steps
    # the step schedule's running product starts again from 1
    opt.reset_state()
    assert float(opt.step_count) == 0.0 and float(opt.last_lr) == base * sch.factor(0)
    assert float(opt._sched_state) == 1.0
    flat.grads[:P].copy_(g_dev[0])
    opt.step()
    assert float(opt.last_lr) == seen[0]
    # and the parameters follow torch's optimizer under a LambdaLR of the same schedule
    _run_against_reference(variant, P, 3, 5e-4, "above", False, schedule_key=key)


def test_constant_rate_is_untouched_by_the_schedule_argument():
    P, sizes = 5000, _segments(5000, 3)
    p0, g = _inputs(P, "off")
    a, b = _Flat(p0, sizes), _Flat(p0, sizes)
    oa = _build("adamW", a, weight_decay=5e-4)
    ob = _build("adamW", b, weight_decay=5e-4, schedule=None)
    g_dev = g.to(DEV)
    for t in range(5):
        for f, o in ((a, oa), (b, ob)):
            f.grads[:P].copy_(g_dev[t])
            o.step()
        assert torch.equal(a.backing, b.backing)
        assert float(oa.last_lr) == float(ob.last_lr) == 1e-2
    ob.set_lr(5e-3)                                        # without a schedule the rate is the caller's
    assert float(ob.last_lr) == 5e-3 and ob.c is not None


@pytest.mark.parametrize("variant,name", [("adagrad_decay", None), ("adamW", "cosine"), ("adagrad", "step_every")])
def test_captured_step_replays_like_eager_steps(variant, name):
    """One step captured on a side stream behind one eager step, replayed 4 times: the twin's 1 + 4 eager steps."""
    P, sizes = 4097, _segments(4097, 5)
    p0, g = _inputs(P, "above")
    sch = None if name is None else _schedule(SCHEDULES[name])
    a, b = _Flat(p0, sizes), _Flat(p0, sizes)
    kw = dict(weight_decay=5e-4, max_norm=MAX_NORM, schedule=sch)
    oa, ob = _build(variant, a, **kw), _build(variant, b, **kw)
    for f in (a, b):
        f.grads[:P].copy_(g[0].to(DEV) * 0.5)               # norm 0.75: the clip leaves the buffer as it is
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        oa.step()
    torch.cuda.synchronize()
    assert float(oa.step_count) == 1.0                     # recorded, not run
    lrs = []
    for _ in range(4):
        graph.replay()
        lrs.append(float(oa.last_lr))
    for _ in range(5):
        ob.step()
    torch.cuda.synchronize()
    assert float(oa.step_count) == float(ob.step_count) == 5.0
    assert torch.equal(a.backing, b.backing)
    assert torch.equal(oa.last_lr, ob.last_lr) and torch.equal(oa.last_norm, ob.last_norm)
    if sch is not None:
        assert lrs == [oa.lr * sch.factor(s) for s in range(1, 5)] if name != "cosine" else \
            all(_within_ulps(l, oa.lr * sch.factor(s)) for l, s in zip(lrs, range(1, 5)))
        assert len(set(lrs)) == 4                          # the rate moves on every replay


# ---- fit_resident --------------------------------------------------------------------------------------------------

def _data(n, seed):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("peptides_func", n, seed=seed)
    rng = np.random.default_rng(seed)
    return [hetero_from_clusters(g, rng.integers(0, 8, g.num_nodes), 8) for g in graphs]


def _model():
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(0)
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(DEV)


@pytest.fixture(scope="module")
def loop_data():
    from graph_hscn.data import DataLoader
    hs = _data(60, 3)
    return hs[:50], [DataLoader(hs[50:55], batch_size=5), DataLoader(hs[55:], batch_size=5)]


def test_fit_resident_adagrad_is_one_launch_inside_the_graph(loop_data):
    """50 graphs in batches of 16 with k = 2 and the clip: iterations 1 and 2 are captured stepping iterations, the
    2-graph tail steps eagerly.  The run with torch's eager Adagrad (``flat_optimizer=False``) is the comparison, at the
    bound tests/test_gpu_pipeline.py uses for FlatAdam against torch -- 2e-4 of the parameter scale (a float64 CPU
    replay of the recorded epoch orders through the oracle model was not built for this test)."""
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.optim import FlatAdagrad
    from graph_hscn.train.train_resident import fit_resident, optimizer_steps_at
    train, loaders = loop_data
    epochs = 3
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=epochs, eval_period=epochs, patience=50)
    cfg = OptimConfig("adagrad", lr=0.05, batch_accumulation=2, clip_grad_norm=True)
    info, orders = {}, []
    model = _model()
    hist = fit_resident(None, cfg, tc, train, loaders, model, batch_size=16, epoch_orders=orders, run_info=info)
    assert isinstance(info["optimizer"], FlatAdagrad)
    assert info["flat"] is True and info["in_graph"] is True and info["schedule"] is None
    nb = 4
    assert float(info["optimizer"].step_count) == epochs * sum(optimizer_steps_at(i, nb, 2) for i in range(nb))
    assert float(info["optimizer"].last_norm) > 0.0        # the clip ran inside the launch
    assert all(np.isfinite(l) for l, _ in hist)
    info2, orders2 = {}, []
    ref = _model()
    fit_resident(None, cfg, tc, train, loaders, ref, batch_size=16, flat_optimizer=False, epoch_orders=orders2,
                 run_info=info2)
    assert isinstance(info2["optimizer"], torch.optim.Adagrad) and info2["in_graph"] is False
    assert all(torch.equal(a, b) for a, b in zip(orders, orders2))     # the same batches in the same order
    worst = max(float((p - q).detach().abs().max()) / max(1.0, float(q.detach().abs().max()))
                for p, q in zip(model.parameters(), ref.parameters()))
    print(f"FlatAdagrad against torch's eager Adagrad after {epochs} epochs: {worst:.3e} of the parameter scale")
    assert worst <= 2e-4


def test_fit_resident_scheduled_adamw_ends_on_the_schedules_last_rate(loop_data):
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.optim import FlatAdam
    from graph_hscn.train.train_resident import fit_resident
    train, loaders = loop_data
    epochs = 4
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=epochs, eval_period=epochs, patience=50)
    cfg = OptimConfig("adamW", scheduler="cosine_with_warmup", warmup_epochs=1)
    info = {}
    hist = fit_resident(None, cfg, tc, train, loaders, _model(), batch_size=16, run_info=info)
    opt, sch = info["optimizer"], info["schedule"]
    assert isinstance(opt, FlatAdam) and info["in_graph"] is True
    assert (sch.warmup_steps, sch.total_steps) == (4, 16)              # 3 captured batches + the tail, k = 1
    assert float(opt.step_count) == sch.total_steps
    lr, want = float(opt.last_lr), cfg.lr * sch.factor(sch.total_steps - 1)
    print(f"last device lr {lr!r}, host {want!r}; losses {[round(l, 5) for l, _ in hist]}")
    assert _within_ulps(lr, want)
    assert hist[-1][0] < hist[0][0]
