"""Learning-rate schedules of the one-launch optimizers, the host side: ``optim.LRSchedule.factor`` against torch's
``LambdaLR``, the config fields and their checks, what ``fit_resident`` refuses before it touches a device, and the C
ABI's argument checks (no launch: runs without a GPU)."""
import ctypes

import pytest
import torch


def _torch_lrs(schedule, base_lr, steps):
    """The rate torch's AdamW holds at every step when a LambdaLR drives it with the schedule's lambda."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([p], lr=base_lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=schedule.as_lambda())
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]["lr"])
        p.grad = torch.ones(3)
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize("kind", ["cosine_with_warmup", "linear_with_warmup"])
@pytest.mark.parametrize("warmup,total", [(0, 1), (1, 2), (3, 10), (10, 10)])
@pytest.mark.parametrize("min_factor", [0.0, 0.05])
def test_warmup_schedules_match_lambda_lr(kind, warmup, total, min_factor):
    from graph_hscn.optim import LRSchedule
    sch = LRSchedule(kind, warmup_steps=warmup, total_steps=total, min_factor=min_factor)
    lrs = _torch_lrs(sch, 0.01, total + 5)
    assert lrs == [0.01 * sch.factor(s) for s in range(total + 5)]
    # the shape of the curve: warm-up from 1e-6 towards 1, the peak at the end of the warm-up, then down to the floor
    assert sch.factor(0) == (1e-6 if warmup else 1.0)
    for s in range(1, warmup):
        assert sch.factor(s) == s / warmup
    if warmup < total:
        assert sch.factor(warmup) == 1.0
    tail = [sch.factor(s) for s in range(warmup, total + 1)]
    assert all(a >= b for a, b in zip(tail, tail[1:]))
    assert all(sch.factor(s) == sch.factor(total) for s in range(total, total + 5))     # clamped behind the end
    if warmup < total:
        assert sch.factor(total) == pytest.approx(min_factor, abs=1e-16)


@pytest.mark.parametrize("period", [1, 4])
def test_step_schedule_matches_lambda_lr(period):
    from graph_hscn.optim import LR_STEP, LRSchedule
    sch = LRSchedule("step", total_steps=10, period=period, gamma=0.7)
    assert sch.kind == LR_STEP
    lrs = _torch_lrs(sch, 0.05, 15)
    assert lrs == [0.05 * sch.factor(s) for s in range(15)]
    for s in range(15):
        assert sch.factor(s) == pytest.approx(0.7 ** (s // period), rel=1e-14)
    assert sch.factor(period - 1) == 1.0 and sch.factor(period) == 0.7


def test_schedule_and_config_validation():
    from graph_hscn.config.config import OptimConfig
    from graph_hscn.optim import LRSchedule
    for bad in (dict(kind="cosine"), dict(kind=0), dict(kind=7), dict(kind="step", period=0),
                dict(kind="step", gamma=0.0), dict(kind="step", gamma=1.5), dict(kind="step", gamma=float("nan")),
                dict(kind="cosine_with_warmup", warmup_steps=5, total_steps=4),
                dict(kind="cosine_with_warmup", warmup_steps=-1, total_steps=4),
                dict(kind="linear_with_warmup", total_steps=4, min_factor=-0.1),
                dict(kind="linear_with_warmup", total_steps=4, min_factor=float("nan"))):
        with pytest.raises(ValueError):
            LRSchedule(**bad)
    cfg = OptimConfig("adamW")                       # the defaults are the reference's constant rate
    assert (cfg.scheduler, cfg.warmup_epochs, cfg.step_epochs, cfg.gamma, cfg.min_lr_factor) == (None, 0, 1, 1.0, 0.0)
    assert OptimConfig("adamW", 2, True, 0.01, 5e-4).lr == 0.01        # the reference's fields keep their places
    OptimConfig("adamW", scheduler="cosine_with_warmup", warmup_epochs=2, min_lr_factor=0.1)
    OptimConfig("adagrad", scheduler="step", step_epochs=3, gamma=0.5)
    for bad in (dict(scheduler="cosine"), dict(scheduler="step", gamma=1.5), dict(scheduler="step", gamma=0.0),
                dict(scheduler="step", gamma=-0.5), dict(scheduler="step", step_epochs=0),
                dict(scheduler="cosine_with_warmup", warmup_epochs=-1),
                dict(scheduler="cosine_with_warmup", min_lr_factor=1.5),
                dict(scheduler="cosine_with_warmup", min_lr_factor=-0.5)):
        with pytest.raises(ValueError):
            OptimConfig("adamW", **bad)


def test_schedule_from_config_counts_optimizer_steps():
    from graph_hscn.config.config import OptimConfig
    from graph_hscn.optim import LR_WARMUP_COSINE, LR_STEP
    from graph_hscn.train.train_resident import optimizer_steps_at, schedule_from_config
    # 7 batches with k = 3 step at iterations 2, 5 and 6: three optimizer steps per epoch
    assert sum(optimizer_steps_at(i, 7, 3) for i in range(7)) == 3
    cfg = OptimConfig("adamW", batch_accumulation=3, lr=0.02, scheduler="cosine_with_warmup", warmup_epochs=2,
                      min_lr_factor=0.1)
    sch = schedule_from_config(cfg, epochs=10, num_batches=7, batch_accumulation=3)
    assert (sch.kind, sch.warmup_steps, sch.total_steps, sch.min_factor, sch.base_lr) == (LR_WARMUP_COSINE, 6, 30, 0.1, 0.02)
    sch = schedule_from_config(OptimConfig("adam", scheduler="step", step_epochs=4, gamma=0.5), 10, 7, 1)
    assert (sch.kind, sch.period, sch.gamma, sch.total_steps) == (LR_STEP, 28, 0.5, 70)
    assert schedule_from_config(OptimConfig("adam"), 10, 7, 1) is None


def test_fit_resident_refuses_a_scheduler_without_the_flat_optimizer_before_the_device():
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.train import train as T
    from graph_hscn.train.train_resident import fit_resident
    model = torch.nn.Linear(2, 2)                    # on the CPU: the device check would raise RuntimeError
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=2)
    cfg = OptimConfig("adamW", scheduler="cosine_with_warmup", warmup_epochs=1)
    with pytest.raises(ValueError, match="flat_optimizer"):
        fit_resident(None, cfg, tc, [None] * 4, [], model, batch_size=2, flat_optimizer=False)
    with pytest.raises(RuntimeError, match="cuda"):  # with the flat optimizer it gets as far as the device check
        fit_resident(None, cfg, tc, [None] * 4, [], model, batch_size=2)
    with pytest.raises(ValueError, match="fit_resident"):      # the reference-shaped loop has no scheduler
        T.train(None, cfg, tc, [[]], model)


def test_flat_optimizer_from_config_takes_adagrad_and_from_config_does_not():
    from graph_hscn.optim import FlatAdam, flat_optimizer_from_config
    flat = torch.zeros(6)
    p = torch.zeros(6)
    views = [(p, flat[:6])]
    assert FlatAdam.from_config("adagrad", views, flat, 0.01, 0.0) is None
    assert flat_optimizer_from_config("sgd", views, flat, 0.01, 0.0) is None
    for name in ("adagrad", "adam", "adamW"):        # the name is taken: construction stops at the device check
        with pytest.raises(RuntimeError, match="HIP device"):
            flat_optimizer_from_config(name, views, flat, 0.01, 0.0)


def test_schedule_record_matches_the_header_and_bad_records_are_refused_before_any_launch():
    from graph_hscn import _hip
    from graph_hscn.optim import LR_CONSTANT, LR_STEP, LR_WARMUP_COSINE, LR_WARMUP_LINEAR, LRSchedule
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hscn.h")).read()
    for name, v in (("CONSTANT", LR_CONSTANT), ("WARMUP_COSINE", LR_WARMUP_COSINE), ("WARMUP_LINEAR", LR_WARMUP_LINEAR),
                    ("STEP", LR_STEP)):
        assert int(re.search(rf"#define HSCN_LR_{name} (\d+)", src).group(1)) == v
    body = re.search(r"typedef struct hscn_lr_schedule \{(.*?)\} hscn_lr_schedule;", src, re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f for f, _ in _hip.LRScheduleC._fields_]
    assert ctypes.sizeof(_hip.LRScheduleC) == 56

    lib = _hip.lib()
    buf = ctypes.create_string_buffer(64)            # stands in for pointers the checks only compare with NULL
    here = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 1)(here)
    off = (ctypes.c_int32 * 2)(0, 4)

    def adam(rec, state=here, P=4):
        return lib.hscn_adam_step_sched(ptrs, off, 1, here, here, here, P, here, here, here, 0.9, 0.999, 1e-8, 0.0, 1,
                                        0.0, None, 0, None if rec is None else ctypes.byref(rec), state, None)

    def adagrad(rec, state=here, P=4):
        return lib.hscn_adagrad_step(ptrs, off, 1, here, here, P, here, here, 0.0, 1e-10, 0.0, 0.0, None, 0,
                                     None if rec is None else ctypes.byref(rec), state, None)

    good = LRSchedule("cosine_with_warmup", warmup_steps=3, total_steps=8, base_lr=0.01).c()
    bad = []
    for field, value in (("kind", 9), ("kind", -1), ("total_steps", 2), ("warmup_steps", -1), ("period", 0),
                         ("gamma", 0.0), ("gamma", 1.5), ("gamma", float("nan")), ("min_factor", -0.5),
                         ("min_factor", float("nan")), ("base_lr", float("nan"))):
        rec = _hip.LRScheduleC.from_buffer_copy(good)
        setattr(rec, field, value)
        bad.append((field, value, rec))
    for call in (adam, adagrad):
        for field, value, rec in bad:
            assert call(rec) == -1, (call.__name__, field, value)           # HSCN_E_BADARG
        assert call(good, state=None) == -1                                  # a schedule needs its running product
        assert call(good, P=0) == 0                                          # nothing to launch
    assert adagrad(None, P=0) == 0 and adam(None, P=0) == 0
    off65 = (ctypes.c_int32 * 66)(*range(66))
    ptrs65 = (ctypes.c_void_p * 65)(*([here] * 65))
    assert lib.hscn_adagrad_step(ptrs65, off65, 65, here, here, 65, here, here, 0.0, 1e-10, 0.0, 0.0, None, 0, None,
                                 None, None) == -3                           # HSCN_E_UNSUPPORTED: 64 tensors at most
    assert lib.hscn_adagrad_step(ptrs, off, 1, here, here, 5, here, here, 0.0, 1e-10, 0.0, 0.0, None, 0, None, None,
                                 None) == -1                                 # the table does not end at P
    assert lib.hscn_adagrad_step(ptrs, off, 1, here, here, 4, here, here, -1.0, 1e-10, 0.0, 0.0, None, 0, None, None,
                                 None) == -1                                 # lr_decay < 0
