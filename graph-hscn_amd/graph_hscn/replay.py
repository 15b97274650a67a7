"""hipGraph replay of the training step across DIFFERENT batches.

A captured step replays only if every pointer and every host-side size it was captured with stays
valid.  The graph-resident kernels read the per-graph node / edge ranges from device arrays, so the
only host constants are capacities: ``StaticHeteroBatch`` owns device buffers sized for the largest
batch of a loader (nodes, edges per relation, virtual nodes; per-graph maxima that size the LDS), each
step's batch is copied INTO them (``load``), and the captured launches run on whatever the buffers
hold.  ``CapturedStep`` captures ``zero grads -> HSCN.forward -> criterion -> backward`` once (as direct C-ABI
launches, ``step.ResidentTrainStep``: no autograd inside the capture); afterwards
a training iteration is ``static.load(batch); step.replay(); optimizer.step()``.

The reference loop (train/train.py:73-95) issues ~150 small launches per step from Python; the eager
path here issues 4 but is still host-bound -- replay is what lets the GPU, not
the interpreter, set the pace of an epoch.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch
from torch import Tensor

from .data import HeteroBatch

LL = ("local", "to", "local")
VV = ("virtual", "to", "virtual")
LV = ("local", "to", "virtual")


class StaticHeteroBatch:
    """Fixed-capacity device buffers with the ``HeteroBatch`` protocol (``.batch`` is the object to hand
    to the model).  Only for the graph-resident engine: edge lists are valid inside the per-graph ranges
    of ``ptr32`` only, the tail of every buffer is stale data of earlier, larger batches.

    All fields are views of ONE flat byte buffer, so a batch that was ``pack``-ed ahead of time (on the
    device or in pinned host memory) is loaded by a single copy."""

    def __init__(self, batches: Iterable[HeteroBatch], device, num_classes: Optional[int] = None,
                 feature_dtype=torch.float32):
        """``feature_dtype``: storage type of the node features in the static buffers (``torch.float16``: the
        half-storage mode of the graph-resident engine; ``load`` converts)."""
        self.feature_dtype = feature_dtype
        batches = list(batches)
        if not batches:
            raise ValueError("need at least one batch to size the buffers")
        B = {int(b.num_graphs) for b in batches}
        if len(B) != 1:
            raise ValueError("all batches must hold the same number of graphs (drop or pad the last one)")
        cap = lambda f: max(int(f(b)) for b in batches)
        y0 = batches[0]["local"].y if "y" in batches[0]["local"] else None
        # class-index targets (one integer per graph): ``y`` is int64 [G]; their C is the model's, not the batch's
        self.class_index = y0 is not None and y0.dim() == 1 and not y0.dtype.is_floating_point
        if y0 is None or self.class_index:
            C = None
        else:
            C = int(y0.size(1)) if num_classes is None else int(num_classes)
        self._allocate(B.pop(), device, cap(lambda b: b["local"].num_nodes), cap(lambda b: b["virtual"].num_nodes),
                       {et: cap(lambda b, et=et: b[et].edge_index.size(1)) for et in (LL, VV, LV)},
                       {"local": cap(lambda b: b["local"].max_nodes), "virtual": cap(lambda b: b["virtual"].max_nodes)},
                       {et: cap(lambda b, et=et: b[et].max_edges) for et in (LL, VV, LV)},
                       int(batches[0]["local"].x.size(1)), C)

    @classmethod
    def from_capacities(cls, num_graphs: int, device, num_nodes: int, num_virtual: int, num_edges: dict,
                        max_nodes: dict, max_edges: dict, num_features: int, num_classes: Optional[int],
                        class_index: bool = False):
        """Buffers for batches of ``num_graphs`` graphs with at most the given totals (nodes, virtual nodes,
        edges per relation) and per-graph maxima (what sizes the LDS of the graph-resident launches).
        ``class_index``: the targets are one int64 class index per graph (``num_classes`` is not used then)."""
        self = cls.__new__(cls)
        self.feature_dtype = torch.float32
        self.class_index = bool(class_index)
        self._allocate(num_graphs, device, num_nodes, num_virtual, num_edges, max_nodes, max_edges, num_features,
                       num_classes)
        return self

    def _allocate(self, G, device, N, V, E, max_nodes, max_edges, F, C):
        self.num_graphs = int(G)
        self.device = torch.device(device)
        self.N, self.V = int(N), int(V)
        self.E = {et: max(int(E[et]), 1) for et in (LL, VV, LV)}
        self.max_nodes = {k: int(v) for k, v in max_nodes.items()}
        self.max_edges = {et: int(max_edges[et]) for et in (LL, VV, LV)}
        fdt = getattr(self, "feature_dtype", torch.float32)
        fields = [("x_local", fdt, (self.N, F)), ("x_virtual", fdt, (self.V, F))]
        for nt, n in (("local", self.N), ("virtual", self.V)):
            fields += [(f"ptr_{nt}", torch.int64, (G + 1,)), (f"ptr32_{nt}", torch.int32, (G + 1,)),
                       (f"batch_{nt}", torch.int64, (n,))]
        if getattr(self, "class_index", False):
            fields.append(("y", torch.int64, (G,)))
        elif C is not None:
            fields.append(("y", torch.float32, (G, C)))
        for i, et in enumerate((LL, VV, LV)):
            fields += [(f"ei_{i}", torch.int64, (2, self.E[et])), (f"eptr_{i}", torch.int32, (G + 1,))]
        self._layout, off = [], 0
        for name, dt, shape in fields:
            nbytes = torch.empty((), dtype=dt).element_size()
            for d in shape:
                nbytes *= d
            self._layout.append((name, dt, shape, off, nbytes))
            off += (nbytes + 15) // 16 * 16
        self.nbytes = off
        self.flat = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.device)
        self.batch = self._view(self.flat)

    def _view(self, flat: Tensor) -> HeteroBatch:
        t = {name: flat[off: off + nb].view(dt).view(shape) for name, dt, shape, off, nb in self._layout}
        hb = HeteroBatch()
        hb.num_graphs = self.num_graphs
        for nt, n in (("local", self.N), ("virtual", self.V)):
            st = hb[nt]
            st.x = t[f"x_{nt}"]
            st.ptr, st.ptr32, st.batch = t[f"ptr_{nt}"], t[f"ptr32_{nt}"], t[f"batch_{nt}"]
            st.num_nodes = n
            st.max_nodes = self.max_nodes[nt]
        if "y" in t:
            hb["local"].y = t["y"]
        for i, et in enumerate((LL, VV, LV)):
            hb[et].edge_index = t[f"ei_{i}"]
            hb[et].ptr32 = t[f"eptr_{i}"]
            hb[et].max_edges = self.max_edges[et]
        return hb

    def _fill(self, dst: HeteroBatch, src: HeteroBatch) -> None:
        if int(src.num_graphs) != self.num_graphs:
            raise ValueError("batch holds a different number of graphs than the static buffers")
        for nt, capn in (("local", self.N), ("virtual", self.V)):
            s, d = src[nt], dst[nt]
            n = int(s.num_nodes)
            if n > capn or int(s.max_nodes) > self.max_nodes[nt]:
                raise ValueError(f"batch exceeds the static capacity of '{nt}' nodes")
            d.x[:n].copy_(s.x, non_blocking=True)
            d.batch[:n].copy_(s.batch, non_blocking=True)
            d.ptr.copy_(s.ptr, non_blocking=True)
            d.ptr32.copy_(s.ptr32, non_blocking=True)
        if "y" in src["local"] and "y" in dst["local"]:
            dst["local"].y.copy_(src["local"].y, non_blocking=True)
        for et in (LL, VV, LV):
            s, d = src[et], dst[et]
            e = int(s.edge_index.size(1))
            if e > self.E[et] or int(s.max_edges) > self.max_edges[et]:
                raise ValueError(f"batch exceeds the static capacity of relation {et}")
            d.edge_index[:, :e].copy_(s.edge_index, non_blocking=True)
            d.ptr32.copy_(s.ptr32, non_blocking=True)

    def pack(self, src: HeteroBatch, device=None, pin_memory: bool = False) -> Tensor:
        """``src`` laid out like the static buffers, as one flat byte tensor (on ``device``, default: the
        static buffers' device; or in pinned host memory): what ``load`` takes with a single copy."""
        dev = torch.device(device) if device is not None else self.device
        flat = torch.zeros(self.nbytes, dtype=torch.uint8, device=dev, pin_memory=(pin_memory and dev.type == "cpu"))
        self._fill(self._view(flat), src)
        return flat

    def load(self, src) -> HeteroBatch:
        """Make the static buffers hold ``src``: a packed byte tensor (one copy) or a ``HeteroBatch`` on the
        host or the device (one copy per field).  Asynchronous on the current stream."""
        if isinstance(src, Tensor):
            if src.dtype != torch.uint8 or src.numel() != self.nbytes:
                raise ValueError("not a batch packed by this StaticHeteroBatch")
            self.flat.copy_(src, non_blocking=True)
        else:
            self._fill(self.batch, src)
        return self.batch


def _snapshot(params, optimizer):
    """Copies of ``params`` and of the tensors in ``optimizer.state`` (none for an optimizer still to be built), for
    ``_restore`` behind the warm-up steps that PyTorch's capture recipe asks for."""
    state = getattr(optimizer, "state", None) or {}
    return ([p.detach().clone() for p in params],
            {id(p): {k: v.clone() for k, v in st.items() if isinstance(v, Tensor)} for p, st in state.items()})


def _restore(params, optimizer, snap) -> None:
    """Put parameters and optimizer state back IN PLACE (captured launches hold their addresses): the old value, or
    zero for state the warm-up created -- the initial state of the Adam family."""
    snap_p, snap_s = snap
    with torch.no_grad():
        for p, s0 in zip(params, snap_p):
            p.copy_(s0)
        if hasattr(optimizer, "reset_state"):          # optim.FlatAdam: built behind the snapshot, all state is new
            optimizer.reset_state()
            return
        for p, st in optimizer.state.items():
            for k, v in st.items():
                if isinstance(v, Tensor):
                    old = snap_s.get(id(p), {}).get(k)
                    v.copy_(old) if old is not None else v.zero_()


def _warm_up_and_capture(fn, warmup: int) -> "torch.cuda.CUDAGraph":
    """PyTorch's capture recipe: ``warmup`` eager calls of ``fn`` on a side stream, then one captured call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def capture_optimizer_step(params, optimizer, warmup: int = 3) -> "torch.cuda.CUDAGraph":
    """``optimizer.step()`` (an optimizer built with ``capturable=True``; ``fused=True`` keeps it to one launch) on
    the gradient buffers ``p.grad`` points at NOW, as a hipGraph of its own.  The warm-up steps PyTorch's capture
    recipe asks for are undone: parameters and optimizer state are put back in place (state the warm-up created is
    zeroed: the initial state of the Adam family)."""
    params = list(params)
    snap = _snapshot(params, optimizer)
    g = _warm_up_and_capture(optimizer.step, warmup)
    _restore(params, optimizer, snap)
    return g


class CapturedStep:
    """``zero grads -> model(batch) -> criterion -> backward`` captured once on ``static.batch``.
    ``replay()`` runs it on whatever was last loaded; ``loss`` / ``pred`` / ``score`` are the captured
    output tensors (refreshed by every replay), parameter gradients are slices of one flat buffer
    (``grads``; ``p.grad`` points into it).

    The captured region holds kernel nodes only: the step is issued through ``step.ResidentTrainStep``
    (direct C-ABI launches on preallocated buffers), never through the autograd engine.  Round 1 captured
    ``loss.backward()``; autograd's gradient-accumulation nodes are bound to the stream of the first step that
    used them, a node kept alive by ANY earlier eager ``loss`` / ``pred`` tied the capture to that
    non-capturing stream and ``capture_end`` died inside the HIP runtime (a host SIGSEGV).  With no autograd
    in the capture, live tensors of earlier eager steps and earlier ``CapturedStep`` objects on the same model
    cannot reach into it (tests/test_gpu_step.py)."""

    def __init__(self, model, static: StaticHeteroBatch, loss_fn: str, warmup: int = 3, optimizer=None, pre=None,
                 one_launch: Optional[bool] = None, reducer=None, structure=None, accumulate: bool = False,
                 max_norm: Optional[float] = None):
        """``one_launch``: passed to ``step.ResidentTrainStep`` (None: the one-launch step whenever the batch fits it;
        False: the forward + backward launch pair, whose gradients are bit-identical to the eager autograd path).
        ``reducer``: a ``distributed.FlatGradReducer``; its all-reduce of the flat gradient buffer (RCCL kernels are
        capturable) is captured between the backward and the optimizer step, so one replay per iteration is all a
        rank issues -- no eager collective launch between replays.  Every rank must hold the same number of graphs
        (``static.num_graphs``): the reduction is the mean over ranks.
        ``structure``: passed to ``step.ResidentTrainStep`` ("batch": the step loads the graphs' CSRs / degree norms
        that ``DeviceHeteroDataset(resident_structure=True)`` gathers with every batch instead of rebuilding them).
        ``pre``: a callable captured in front of the step that refreshes the static buffers from device-side
        state only (``DeviceHeteroDataset.gather_next``); note that the warm-up iterations and the capture call
        it too (rewind with ``new_epoch`` afterwards).
        ``optimizer``: a ``torch.optim`` optimizer built with ``capturable=True`` (``fused=True`` keeps it to two
        launches), or a callable ``step -> optim.FlatAdam`` (built on the step's flat gradient buffer: ONE launch;
        afterwards ``self.optimizer``); its ``step()`` is captured behind the backward, so a replay is a whole
        training iteration.
        The ``warmup`` eager iterations that precede the capture run the optimizer too (PyTorch's whole-network
        capture recipe); parameters and optimizer state are put back afterwards, IN PLACE (the captured launches
        hold their addresses): state that existed before is restored, state the warm-up created is zeroed (the
        initial state of the Adam family).
        ``accumulate`` (the reference's ``batch_accumulation``, train/train.py:89-95): the step ADDS its gradients to
        the flat buffer (``ResidentTrainStep(accumulate=True)``) and two graphs share every buffer: ``graph`` (the
        boundary iteration: gather, step, all-reduce, clip, optimizer step, gradients zeroed -- by the optimizer's
        own launch when it is an ``optim.FlatAdam(zero_grads=True)``) and ``micro_graph`` (gather and step only,
        captured without warm-up runs of its own: parameters, optimizer state and the gather's counter end up as with
        one capture).  ``replay(step_optimizer=False)`` replays the micro graph.  Without an optimizer both would be
        the same graph: ``micro_graph`` is then ``graph`` and zeroing is the caller's.
        ``max_norm``: ``clip_grad_norm_`` of the flat gradient between the all-reduce and the optimizer step as a
        launch of its own (``optim.clip_grad_norm_flat``; ``clip_norm`` receives the pre-clip norm), for an
        optimizer that is not a clipping ``FlatAdam``.
        With neither, the one graph captured is the one captured before these modes existed."""
        from .optim import clip_grad_norm_flat
        from .train.batching import resident_step
        self.model, self.static, self.loss_fn, self.optimizer = model, static, loss_fn, optimizer
        params = list(model.parameters())
        snap = _snapshot(params, optimizer) if optimizer is not None else None
        self.step = resident_step(model, static.batch, loss_fn, one_launch, structure, accumulate)
        self.step.bind_grads()
        model.last_engine = "resident"
        if callable(optimizer) and not hasattr(optimizer, "step"):     # ``lambda step: optim.FlatAdam(...)``: built
            optimizer = self.optimizer = optimizer(self.step)          # here, on the step's flat gradient buffer

        pre_args = (self.step,)      # ``gather_next(step)``; () once ``pre`` has turned out to take no argument

        P = self.step.P
        self.accumulate = bool(accumulate)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.clip_norm = torch.full((1,), float("nan"), dtype=torch.float32, device=static.device) \
            if self.max_norm is not None else None
        zero_after = self.accumulate and optimizer is not None and not getattr(optimizer, "zero_grads", False)

        def step(boundary: bool = True):
            nonlocal pre_args
            if pre is not None:
                try:
                    pre(*pre_args)
                except TypeError as e:
                    if not pre_args or e.__traceback__.tb_next is not None:     # (raised inside ``pre``)
                        raise
                    pre_args = ()
                    pre()
            self.step.run()
            if not boundary:
                return
            if reducer is not None:
                reducer.reduce(float(static.num_graphs), float(static.num_graphs * reducer.world_size))
            if self.max_norm is not None:
                clip_grad_norm_flat(self.step.grads[:P], self.max_norm, self.clip_norm)
            if optimizer is not None:
                optimizer.step()
            if zero_after:
                self.step.grads[:P].zero_()

        self.graph = _warm_up_and_capture(step, warmup)
        self.micro_graph = self.graph
        if self.accumulate and (optimizer is not None or reducer is not None or self.max_norm is not None):
            self.micro_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.micro_graph):     # (recorded, not run: nothing to undo)
                step(boundary=False)
        self.pred, self.loss, self.score = self.step.pred, self.step.loss, self.step.score
        # the gradient tensors the captured backward writes (a later eager step re-points ``p.grad`` elsewhere)
        self.grads = list(self.step.param_grads)
        if optimizer is not None:
            _restore(params, optimizer, snap)
        if self.accumulate:        # the first micro-batch adds onto zeros, not onto the warm-up's gradients
            self.step.grads.zero_()
        if self.clip_norm is not None:
            self.clip_norm.fill_(float("nan"))

    def replay(self, step_optimizer: bool = True) -> Tensor:
        """One iteration on the next batch.  ``step_optimizer=False`` (with ``accumulate``): the micro graph --
        the batch's gradients are added to the flat buffer, nothing else."""
        (self.graph if step_optimizer else self.micro_graph).replay()
        return self.loss

    def bind_grads(self) -> None:
        """Point every ``p.grad`` at the captured step's gradient buffers again (after eager steps of the same
        model): an optimizer stepped OUTSIDE the graph reads ``p.grad``."""
        self.step.bind_grads()
