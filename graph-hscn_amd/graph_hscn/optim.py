"""``torch.optim.Adam`` / ``AdamW`` behind a resident training step, as ONE launch.

The reference builds its optimizer from ``OPTIM_DICT`` (config/config.py:24-28; train/train.py:82,
train/train_clustering.py:30-33) and calls ``optimizer.step()`` after every backward.  The resident steps
(``step.ResidentTrainStep`` / ``step.ScnTrainStep``) leave all parameter gradients in ONE flat buffer; ``FlatAdam``
applies torch's single-tensor Adam / AdamW update to the module's own parameter tensors from that buffer with one
launch (``hscn_adam_step``, csrc/optim.hip) where torch's capturable fused optimizer takes two (8.6 us of kernel
time behind a 21 us stage-A step).  Same formulas, operation for operation; the state lives in flat buffers
(``exp_avg``, ``exp_avg_sq``, a float ``step`` counter and the learning rate, all on the device: the launch is
capturable; ``set_lr`` rewrites ``lr`` between launches, an ``LRSchedule`` moves it inside them).

The two optimizer-side settings of the reference's loop (train/train.py:89-95) ride on the same launch
(``hscn_adam_step_ex``): ``max_norm`` is ``nn.utils.clip_grad_norm_(params, max_norm)`` in front of the update, and
``zero_grads`` the ``optimizer.zero_grad()`` behind it that gradient accumulation needs.  ``clip_grad_norm_flat`` is
the clip as a launch of its own, for optimizers that are not this one.

``FlatAdagrad`` is ``torch.optim.Adagrad`` (the third member of ``OPTIM_DICT``) on the same flat layout and with the
same surface (``hscn_adagrad_step``: one launch, clip and zeroing in it), and ``LRSchedule`` a learning-rate schedule
that both evaluate INSIDE their launch from the device step counter (``hscn_adam_step_sched``): warm-up + cosine,
warm-up + linear or step decay with no ``set_lr`` between two replays of a captured iteration.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _hip


class _AdamC(ctypes.Structure):        # include/hscn.h: hscn_adam
    _fields_ = [("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("step", ctypes.c_void_p),
                ("beta_pows", ctypes.c_void_p), ("lr", ctypes.c_void_p), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double),
                ("decoupled", ctypes.c_int)]


LR_CONSTANT, LR_WARMUP_COSINE, LR_WARMUP_LINEAR, LR_STEP = 0, 1, 2, 3     # include/hscn.h: HSCN_LR_*
SCHEDULE_KINDS = {"cosine_with_warmup": LR_WARMUP_COSINE, "linear_with_warmup": LR_WARMUP_LINEAR, "step": LR_STEP}


@dataclass
class LRSchedule:
    """``hscn_lr_schedule`` (include/hscn.h): the learning rate of the optimizer step behind ``s`` completed steps is
    ``base_lr * factor(s)``.  ``kind``: ``LR_WARMUP_COSINE`` / ``LR_WARMUP_LINEAR`` / ``LR_STEP`` or their
    ``OptimConfig.scheduler`` names; all lengths in optimizer steps.  ``base_lr=None``: the ``lr`` of the optimizer
    the schedule is handed to."""
    kind: Union[int, str]
    warmup_steps: int = 0
    total_steps: int = 0
    period: int = 1
    gamma: float = 1.0
    min_factor: float = 0.0
    base_lr: Optional[float] = None

    def __post_init__(self):
        if isinstance(self.kind, str):
            if self.kind not in SCHEDULE_KINDS:
                raise ValueError(f"unknown schedule {self.kind!r} (one of {sorted(SCHEDULE_KINDS)})")
            self.kind = SCHEDULE_KINDS[self.kind]
        if self.kind not in (LR_WARMUP_COSINE, LR_WARMUP_LINEAR, LR_STEP):
            raise ValueError(f"unknown schedule kind {self.kind!r}")
        self.warmup_steps, self.total_steps, self.period = int(self.warmup_steps), int(self.total_steps), int(self.period)
        self.gamma, self.min_factor = float(self.gamma), float(self.min_factor)
        if self.warmup_steps < 0 or self.total_steps < self.warmup_steps:
            raise ValueError("a schedule needs 0 <= warmup_steps <= total_steps")
        if self.period < 1:
            raise ValueError("period must be at least 1")
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError("gamma must be in (0, 1]")
        if not self.min_factor >= 0.0:
            raise ValueError("min_factor must be non-negative")
        if self.base_lr is not None and not float(self.base_lr) >= 0.0:
            raise ValueError("base_lr must be non-negative")

    def factor(self, s: int) -> float:
        """The host twin of the device formula (csrc/optim.hip: sched_lr), operation for operation in Python floats."""
        s = int(s)
        if self.kind == LR_STEP:
            f = 1.0
            for _ in range(s // self.period):     # the running product the device keeps, not gamma ** n
                f = f * self.gamma
            return f
        w, T = self.warmup_steps, self.total_steps
        if s < w:
            return max(1e-6, s / max(1, w))
        s = min(s, T)
        span = max(1, T - w)
        if self.kind == LR_WARMUP_COSINE:
            return max(self.min_factor, 0.5 * (1.0 + math.cos(math.pi * (s - w) / span)))
        return max(self.min_factor, (T - s) / span)

    def as_lambda(self) -> Callable[[int], float]:
        """For ``torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=...)``: the same schedule on a torch optimizer."""
        return self.factor

    def c(self) -> "_hip.LRScheduleC":
        if self.base_lr is None:
            raise ValueError("the schedule has no base_lr yet")
        return _hip.LRScheduleC(int(self.kind), float(self.base_lr), self.warmup_steps, self.total_steps, self.period,
                                self.gamma, self.min_factor)


class _FlatOptimizer:
    """What the one-launch optimizers share: the parameter tensors tile the front of one flat gradient buffer, their
    pointers and offsets travel as host tables, the learning rate is a device word (a schedule's launch rewrites it),
    and the clip / zeroing settings ride on the update's launch."""

    MAX_PARAMS = 64

    def _init_flat(self, param_grads: Sequence[Tuple[Tensor, Tensor]], flat_grads: Tensor, lr: float,
                   max_norm: Optional[float], zero_grads: bool, schedule: Optional[LRSchedule]) -> None:
        name = type(self).__name__
        if not param_grads or len(param_grads) > self.MAX_PARAMS:
            raise ValueError(f"{name} takes 1..{self.MAX_PARAMS} parameter tensors")
        if flat_grads.dtype != torch.float32 or not flat_grads.is_contiguous():
            raise ValueError("the flat gradient buffer must be contiguous float32")
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError("max_norm must be positive")
        if schedule is not None and schedule.base_lr is None:
            schedule = dataclasses.replace(schedule, base_lr=float(lr))
        dev = flat_grads.device
        if dev.type != "cuda":
            raise RuntimeError(f"{name} runs on the HIP device only: the flat gradient buffer is on {dev}")
        base, off, offs = flat_grads.data_ptr(), 0, [0]
        for p, g in param_grads:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("parameters must be contiguous float32 tensors on the gradient buffer's device")
            if g.data_ptr() != base + 4 * off or g.numel() != p.numel():
                raise ValueError("param_grads must tile the front of the flat gradient buffer in order")
            off += p.numel()
            offs.append(off)
        self.param_grads = list(param_grads)
        self.params = [p for p, _ in param_grads]
        self.P = off
        self.grads = flat_grads
        self._ptr_list = [p.data_ptr() for p in self.params]
        self._ptrs = (ctypes.c_void_p * len(self.params))(*self._ptr_list)      # host tables: kernel arguments
        self._off = (ctypes.c_int32 * len(offs))(*offs)
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        self.schedule = schedule
        self.lr = float(lr) if schedule is None else float(schedule.base_lr)
        self._lr = torch.tensor([self._initial_lr()], dtype=torch.float64, device=dev)
        self.last_lr = self._lr.view(())          # the rate of the last step (of the next one before the first)
        self._sched_c = None if schedule is None else schedule.c()
        self._sched_ref = None if schedule is None else ctypes.byref(self._sched_c)
        # gamma^floor(s / period) of a step schedule: a running product on the device, like Adam's beta powers
        self._sched_state = None if schedule is None else torch.ones(1, dtype=torch.float64, device=dev)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.zero_grads = bool(zero_grads)
        self._norm = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        self.last_norm = self._norm.view(())      # pre-clip norm of the last step (NaN before a clipped step)

    def _initial_lr(self) -> float:
        return self.lr if self.schedule is None else self.schedule.base_lr * self.schedule.factor(0)

    def _reset_flat(self) -> None:
        self.step_count.zero_()
        self._norm.fill_(float("nan"))
        if self.schedule is not None:
            self._lr.fill_(self._initial_lr())
            self._sched_state.fill_(1.0)

    def set_lr(self, lr: float) -> None:
        """A new learning rate (one tiny copy; the captured launch reads the device value).  With a schedule the
        launch itself owns the rate."""
        if self.schedule is not None:
            raise RuntimeError("the optimizer was built with a schedule, which owns the learning rate")
        self.lr = float(lr)
        self._lr.fill_(self.lr)

    def step_from_autograd(self, accumulate: bool = False) -> None:
        """A step on the gradients an EAGER backward left in ``p.grad`` (an epoch's ragged last batch runs through
        autograd): copied into the flat buffer first (parameters without a gradient contribute zeros, as torch's
        optimizers skip them only when ALL their history is empty -- here they have none either: the resident
        steps never produce a gradient for them and they are not in ``params``).
        ``accumulate``: ADDED to what the flat buffer holds instead (the earlier micro-batches of an accumulation
        window: autograd's ``p.grad += new``)."""
        self.collect_autograd(accumulate)
        self.step()

    def collect_autograd(self, accumulate: bool = False) -> None:
        """The first half of ``step_from_autograd``: ``p.grad`` into the flat buffer (copied, or added with
        ``accumulate``), no step."""
        collect_autograd(self.param_grads, accumulate)

    def check(self) -> None:
        """The parameter tensors are still the ones the pointer table was built from (``module.to()`` / a loaded
        checkpoint that re-allocates them would leave the launch updating dead memory)."""
        if self._ptr_list != [p.data_ptr() for p in self.params]:
            raise RuntimeError(f"a parameter tensor was re-allocated after {type(self).__name__} was built")

    def zero_grad(self, set_to_none: bool = True) -> None:
        """For an EAGER backward (the resident steps overwrite the flat buffer and need none of this): drop the
        parameters' ``.grad`` (autograd then allocates fresh ones; ``step_from_autograd`` collects them) or zero them."""
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()


class FlatAdam(_FlatOptimizer):
    """``param_grads``: ``[(parameter, view of its gradient inside flat_grads)]`` in flat order -- what
    ``ResidentTrainStep.param_grads`` / ``ScnTrainStep.param_grads`` hold.  ``decoupled=True`` is ``AdamW``.
    ``amsgrad`` / ``maximize`` are not offered (the reference never sets them)."""

    def __init__(self, param_grads: Sequence[Tuple[Tensor, Tensor]], flat_grads: Tensor, lr: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 decoupled: bool = False, max_norm: Optional[float] = None, zero_grads: bool = False,
                 schedule: Optional[LRSchedule] = None):
        """``max_norm``: clip the flat gradient to this 2-norm before every update (torch's ``clip_grad_norm_``;
        ``last_norm`` receives the pre-clip norm, the clipped gradient is left in the buffer).  ``zero_grads``: zero
        the flat gradient buffer after every update (the next accumulating backward adds onto zeros).
        ``schedule``: the launch forms the step's rate from the device step counter (``hscn_adam_step_sched``) and
        leaves it in ``last_lr``; ``lr`` is the schedule's base rate unless it names its own."""
        self._init_flat(param_grads, flat_grads, lr, max_norm, zero_grads, schedule)
        dev = flat_grads.device
        self.betas, self.eps, self.weight_decay, self.decoupled = (float(betas[0]), float(betas[1])), float(eps), \
            float(weight_decay), bool(decoupled)
        self.exp_avg = torch.zeros(self.P, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.P, dtype=torch.float32, device=dev)
        self._beta_pows = torch.ones(2, dtype=torch.float64, device=dev)      # beta1^t, beta2^t (running products)

    @property
    def c(self) -> _AdamC:
        """The state as ``hscn_adam`` (for a step that applies the update in its own launch:
        ``ScnTrainStep.run(opt=...)``).  Those launches read the device ``lr`` word and know no schedule."""
        if self.schedule is not None:
            raise RuntimeError("a scheduled FlatAdam cannot be applied inside a step's own launch (hscn_adam has no "
                               "schedule): build it without one")
        if not hasattr(self, "_c"):
            self._c = _AdamC(_hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq), _hip.ptr(self.step_count),
                             _hip.ptr(self._beta_pows), _hip.ptr(self._lr), self.betas[0], self.betas[1], self.eps,
                             self.weight_decay, int(self.decoupled))
        return self._c

    def step(self) -> None:
        """One optimizer step on the gradients the flat buffer holds NOW (clipped first / zeroed afterwards when the
        optimizer was built so).  Asynchronous, capturable."""
        if self.schedule is not None:
            _hip.call("hscn_adam_step_sched", self._ptrs, self._off, len(self.params), _hip.ptr(self.grads),
                      _hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq), self.P, _hip.ptr(self.step_count),
                      _hip.ptr(self._beta_pows), _hip.ptr(self._lr), self.betas[0], self.betas[1], self.eps,
                      self.weight_decay, int(self.decoupled), self.max_norm or 0.0, _hip.ptr(self._norm),
                      int(self.zero_grads), self._sched_ref, _hip.ptr(self._sched_state), _hip.stream())
            return
        if self.max_norm is not None or self.zero_grads:
            _hip.call("hscn_adam_step_ex", self._ptrs, self._off, len(self.params), _hip.ptr(self.grads),
                      _hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq), self.P, _hip.ptr(self.step_count),
                      _hip.ptr(self._beta_pows), _hip.ptr(self._lr), self.betas[0], self.betas[1], self.eps,
                      self.weight_decay, int(self.decoupled), self.max_norm or 0.0, _hip.ptr(self._norm),
                      int(self.zero_grads), _hip.stream())
            return
        _hip.call("hscn_adam_step", self._ptrs, self._off, len(self.params), _hip.ptr(self.grads),
                  _hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq), self.P, _hip.ptr(self.step_count),
                  _hip.ptr(self._beta_pows), _hip.ptr(self._lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, int(self.decoupled),
                  _hip.stream())

    def reset_state(self) -> None:
        """Back to the state of a freshly built optimizer (moments and step counter zero; a schedule back at step 0,
        its running product at 1), in place."""
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self._beta_pows.fill_(1.0)
        self._reset_flat()

    @classmethod
    def from_config(cls, optim_type: str, param_grads, flat_grads, lr: float, weight_decay: float, **kw):
        """The reference's ``OPTIM_DICT[optim_type](params, lr=..., weight_decay=...)`` for the two members this
        class covers ("adam", "adamW"); None for the others (the caller keeps the torch optimizer)."""
        if optim_type == "adam":
            return cls(param_grads, flat_grads, lr=lr, weight_decay=weight_decay, decoupled=False, **kw)
        if optim_type == "adamW":
            return cls(param_grads, flat_grads, lr=lr, weight_decay=weight_decay, decoupled=True, **kw)
        return None


class FlatAdagrad(_FlatOptimizer):
    """``torch.optim.Adagrad`` with ``FlatAdam``'s surface: one launch (``hscn_adagrad_step``) on the flat gradient
    buffer, capturable, clip / zeroing / schedule in it.  The state is ``state_sum`` (filled with
    ``initial_accumulator_value``) and the float step counter.  ``maximize`` is not offered."""

    def __init__(self, param_grads: Sequence[Tuple[Tensor, Tensor]], flat_grads: Tensor, lr: float = 1e-2,
                 lr_decay: float = 0.0, eps: float = 1e-10, weight_decay: float = 0.0,
                 initial_accumulator_value: float = 0.0, max_norm: Optional[float] = None, zero_grads: bool = False,
                 schedule: Optional[LRSchedule] = None):
        if not float(lr_decay) >= 0.0 or not float(initial_accumulator_value) >= 0.0:
            raise ValueError("lr_decay and initial_accumulator_value must be non-negative")
        self._init_flat(param_grads, flat_grads, lr, max_norm, zero_grads, schedule)
        self.lr_decay, self.eps, self.weight_decay = float(lr_decay), float(eps), float(weight_decay)
        self.initial_accumulator_value = float(initial_accumulator_value)
        self.state_sum = torch.full((self.P,), self.initial_accumulator_value, dtype=torch.float32,
                                    device=flat_grads.device)

    def step(self) -> None:
        """One optimizer step on the gradients the flat buffer holds NOW.  Asynchronous, capturable."""
        _hip.call("hscn_adagrad_step", self._ptrs, self._off, len(self.params), _hip.ptr(self.grads),
                  _hip.ptr(self.state_sum), self.P, _hip.ptr(self.step_count), _hip.ptr(self._lr), self.lr_decay,
                  self.eps, self.weight_decay, self.max_norm or 0.0, _hip.ptr(self._norm), int(self.zero_grads),
                  self._sched_ref, _hip.ptr(self._sched_state), _hip.stream())

    def reset_state(self) -> None:
        """Back to the state of a freshly built optimizer, in place."""
        self.state_sum.fill_(self.initial_accumulator_value)
        self._reset_flat()


FLAT_OPTIMIZERS = ("adam", "adamW", "adagrad")


def flat_optimizer_from_config(optim_type: str, param_grads, flat_grads, lr: float, weight_decay: float, **kw):
    """The reference's ``OPTIM_DICT[optim_type](params, lr=..., weight_decay=...)`` as a one-launch optimizer:
    ``FlatAdam`` for "adam" / "adamW", ``FlatAdagrad`` for "adagrad", None for a name outside ``OPTIM_DICT``."""
    if optim_type == "adagrad":
        return FlatAdagrad(param_grads, flat_grads, lr=lr, weight_decay=weight_decay, **kw)
    return FlatAdam.from_config(optim_type, param_grads, flat_grads, lr, weight_decay, **kw)


def collect_autograd(param_grads: Sequence[Tuple[Tensor, Tensor]], accumulate: bool = False) -> None:
    """``p.grad`` of an eager backward into ``g`` for every ``(p, g)``: copied (zeros for a parameter without a
    gradient), or added with ``accumulate``; a ``p.grad`` that already is ``g`` is left alone."""
    with torch.no_grad():
        for p, g in param_grads:
            if p.grad is None:
                if not accumulate:
                    g.zero_()
            elif p.grad.data_ptr() != g.data_ptr():
                g.add_(p.grad.view_as(g)) if accumulate else g.copy_(p.grad.view_as(g))


def clip_grad_norm_flat(flat_grads: Tensor, max_norm: float, norm_out: Optional[Tensor] = None) -> None:
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` on parameters whose gradients tile ``flat_grads``
    (contiguous float32, on the device), in place, as one launch (``hscn_clip_grad_norm_flat``: the norm and the
    scaling of ``hscn_adam_step_ex``).  ``norm_out`` (float32, >= 1 element) receives the pre-clip norm -- torch's
    return value.  Asynchronous, capturable."""
    if flat_grads.dtype != torch.float32 or not flat_grads.is_contiguous():
        raise ValueError("the flat gradient buffer must be contiguous float32")
    if norm_out is not None and (norm_out.dtype != torch.float32 or norm_out.device != flat_grads.device):
        raise ValueError("norm_out must be a float32 tensor on the gradient buffer's device")
    _hip.call("hscn_clip_grad_norm_flat", _hip.ptr(flat_grads), flat_grads.numel(), float(max_norm),
              _hip.ptr(norm_out), _hip.stream())
