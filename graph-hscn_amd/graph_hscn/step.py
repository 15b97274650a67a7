"""Training steps as plain sequences of C-ABI launches on preallocated buffers (no autograd inside).

The reference's iteration is ``pred = model(...); loss = criterion(...); loss.backward()``
(/root/reference/graph_hscn/train/train.py:73-95; stage A: train/train_clustering.py:44-50).  The
eager product path keeps that form (``engine.HSCNResidentFn`` / ``SCNResidentFn`` are autograd
Functions).  A step that is going to be REPLAYED (hipGraph) should not run the autograd engine while
it is being captured: autograd binds every parameter's gradient-accumulation node to the stream it
was first used on, and a node that an earlier eager step left alive ties the capture to that
non-capturing stream -- ``capture_end`` then fails inside the HIP runtime (a host segfault, round 1:
gpurun_out/t12.log, scn_dbg.log).  The classes here issue exactly the launches the autograd path
issues -- through the same ``engine.launch_*`` builders, so same entry points and same arguments by
construction, and bit-identical outputs (tests/test_gpu_step.py) -- into buffers allocated once, so
a capture contains kernel nodes only and nothing of an earlier step can reach into it.

  ResidentTrainStep  stage C: zero grads -> HSCN.forward -> criterion -> backward
  ScnTrainStep       stage A: zero grads -> gcn_norm + SCN.forward -> (mc + o).backward
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _hip
from . import engine as _engine
from ._hip import call, ptr, stream

LL, VV, LV = _engine.LL, _engine.VV, _engine.LV


def _loss_kind(loss_fn: str, C_pred: Tuple[int, int], target: Tensor) -> int:
    if target.dim() != 2 or tuple(target.shape) != tuple(C_pred):
        raise ValueError("the fused step takes [B, C] targets (the multilabel BCE / L1 branches of "
                         "loss.py:8-10,16-19); class-index targets go through loss.criterion")
    return 0 if loss_fn == "cross_entropy" else 1


class _FlatGradStep:
    def bind_grads(self) -> None:
        """Point every ``p.grad`` at its slice of ``grads``; the model's other parameters get ``None``, as autograd
        leaves them."""
        has = {id(p) for p, _ in self.param_grads}
        for p in self.model.parameters():
            if id(p) not in has:
                p.grad = None
        for p, g in self.param_grads:
            p.grad = g


class ResidentTrainStep(_FlatGradStep):
    """``for p: p.grad = None; pred = model(x_dict, edge_index_dict, batch); loss, score =
    criterion(loss_fn, pred, batch["local"].y); loss.backward()`` on the graph-resident engine,
    issued by ``run()`` as two or three launches on the current stream.

    Class-index targets (``loss_fn="cross_entropy"`` with a contiguous int64 ``[B]`` target on the device: the
    criterion's multiclass branch, loss.py:11-14) run as THREE launches: the forward launch of the pair,
    ``hscn_softmax_nll_fwd`` on its prediction (loss, log-probabilities, dL/dpred), and the backward launch on that
    dense ``g_pred`` with no loss tail.  ``score`` then holds the log-probabilities, ``loss`` is a buffer of its own
    (the backward launch without a tail writes the ``P`` parameter columns of ``grads`` only), and a class index
    outside ``[0, C)`` sets a bit in ``class_flags`` that ``check()`` turns into ``IndexError``.  The one-launch step
    has no class-index loss row: ``one_launch=None`` resolves to this form, ``one_launch=True`` raises.

    Outputs (tensors that every ``run()`` refreshes in place): ``pred`` [B,C], ``score`` [B,C]
    (= sigmoid(pred), what ``criterion`` returns beside the loss), ``loss`` (0-dim), ``grads``
    (flat, the parameter gradients in launch order) and ``virtual`` (final virtual features, as
    ``HSCN.last_virtual``).  ``bind_grads()`` points every ``p.grad`` at its slice of ``grads``
    (parameters the prediction does not depend on -- the whole virtual branch, DESIGN.md section 2 --
    get ``None``, as autograd leaves them).

    The batch may be a ``replay.StaticHeteroBatch.batch``: tensor shapes are capacities then, the
    kernels read the real per-graph ranges from the device-side segment tables."""

    def __init__(self, model, batch, loss_fn: str, target: Optional[Tensor] = None, one_launch: Optional[bool] = None,
                 structure=None, accumulate: bool = False):
        """``one_launch``: None = take the one-launch step (include/hscn.h: hscn_resident_train_step -- forward, loss
        tail and backward of a graph in one workgroup, nothing exported in between) whenever the graphs fit it,
        else the forward + backward launch pair; False = always the pair; True = insist (raises if unsupported).
        ``structure``: None = every step rebuilds the graphs' CSRs and degree norms in LDS from the COO slices
        (structure_build "per-step"); an ``engine.BatchStructure`` (or "batch" = ``batch.structure``, which
        ``engine.build_structure`` / ``DeviceHeteroDataset(resident_structure=True)`` attach) = the one-launch step
        loads them (structure_build "dataset-resident": graph structure is epoch-invariant).  Same results.
        ``accumulate``: gradient accumulation (the reference's ``batch_accumulation``, train/train.py:89-95): the
        step's gradient fold ADDS to ``grads`` (include/hscn.h: HSCN_GRAD_ACCUMULATE -- the same launches), so
        k runs leave ``((g1 + g2) + ...) + gk`` there, autograd's ``p.grad += new``; ``loss`` is still the loss of the
        last run.  Whoever steps the optimizer zeroes ``grads`` afterwards (``optim.FlatAdam(zero_grads=True)``)."""
        from .model.hscn import HSCN, _act_name
        if not isinstance(model, HSCN):
            raise TypeError("ResidentTrainStep drives graph_hscn.model.hscn.HSCN")
        model._refuse_node_level("ResidentTrainStep (hscn_resident_*)")
        model._refuse_vl("ResidentTrainStep (hscn_resident_*)")
        x_dict, ei_dict = batch.x_dict, batch.edge_index_dict
        dev = x_dict["local"].device
        if dev.type != "cuda":
            raise RuntimeError("the graph-resident step runs on the MI355X HIP path: move the batch to 'cuda'")
        keep = model.engine
        model.engine = "resident"            # raises with the reason when the batch / model does not qualify
        try:
            meta, act_name = model._resident_plan(x_dict, ei_dict, batch)
        finally:
            model.engine = keep
        self.model, self.batch, self.meta = model, batch, meta
        self.loss_fn = loss_fn
        params = [p.contiguous() for p in model._resident_params()]
        L = (len(params) - 4) // 9
        W1, b1, W2, b2 = params[9 * L:]
        H, C = W1.shape[0], W2.shape[0]
        self.x_local = x_dict["local"].contiguous()
        self.x_virtual = x_dict["virtual"].contiguous()
        sdt = self.x_local.dtype        # storage type of features and activations (include/hscn.h: HSCN_STORE_F16)
        if sdt not in (torch.float32, torch.float16) or self.x_virtual.dtype != sdt:
            raise TypeError("node features must be float32 (train/train.py:79 casts them) or float16, local and "
                            "virtual alike")
        self._store = _engine.storage_flag(sdt)
        self.accumulate = bool(accumulate)
        # (the gradient-producing launch also carries the accumulation flag)
        self._grad_flags = self._store | (_hip.GRAD_ACCUMULATE if self.accumulate else 0)
        self.ei = {k: ei_dict[k].contiguous() for k in (LL, VV, LV)}
        N, F = self.x_local.shape
        V = self.x_virtual.shape[0]
        B = meta.num_graphs
        self.dims = (N, V, F, H, L, C, B)
        self.head_act = _engine.ACT[act_name]
        self.slope = float(model.convs[0].convs["__".join(LV)].negative_slope)
        y = target if target is not None else batch["local"].y
        self.class_index = bool(loss_fn == "cross_entropy" and y.dim() == 1 and y.dtype == torch.int64
                                and y.is_contiguous() and y.device == dev)
        if self.class_index:
            if y.size(0) != B:
                raise ValueError("class-index targets are one int64 per graph: [B]")
            if one_launch:
                raise RuntimeError("the one-launch step has no class-index loss row: class-index targets run as the "
                                   "forward launch, hscn_softmax_nll_fwd and the backward launch (one_launch=None)")
            one_launch = False
            self.kind = None
        else:
            if y.dtype != torch.float32 or not y.is_contiguous() or y.device != dev:
                raise TypeError("targets must be a contiguous float32 tensor on the batch's device")
            self.kind = _loss_kind(loss_fn, (B, C), y)
        self.target = y
        self._head = params[9 * L:]
        self._table = _engine._ptr_table(params[: 9 * L])
        self._wll_table = _engine._ptr_table([params[9 * l] for l in range(L)])
        # the virtual branch rides on the two launches as extra workgroups while they land on idle CUs
        self.defer = _engine.defers_virtual(model.compute_virtual, model.overlap_virtual, self.dims, dev)
        self._out, self._state = _engine.hscn_buffers(dev, sdt, self.dims, *(self.ei[k].size(1) for k in (LL, LV, VV)),
                                                      score=not self.class_index, csr=True, state=self.defer)
        self.acts, self.pooled, self.z, self.pred, self.score, self.csr = self._out
        self.virtual = torch.empty(max(V, 1), H, dtype=sdt, device=dev) if model.compute_virtual else None
        cus = _engine._cu_count(dev)
        # the one-launch step's virtual workgroups also fit beside small graphs' 4-wave workgroups (several per CU)
        per_cu = int(_hip.lib().hscn_resident_train_step_wgs_per_cu(F, H, L, C, meta.max_n, meta.max_ell, meta.max_v,
                                                                    meta.max_evv))
        # ... and, H = 16, at ANY batch size: 2 B workgroups then take several rounds of the chip, local programs first
        # (block ids [0, B)), so a virtual workgroup's producer has always been dispatched before it; measured against the
        # launch pair at B = 256 / 512 / 1024: 47.9 / 86.2 / 163 us against 56.5 / 105 / 193 (profiles/r03_large_batches.txt).
        # (graphs of the 4-wave class, n <= 64, keep the rule: PCQM-Contact at B = 2 048 / 4 096 runs 101 / 183 us as the
        # launch pair against 116 / 217)
        large_b = H == 16 and meta.max_n > 64
        self.idle_cus = bool(model.compute_virtual and model.overlap_virtual and V > 0 and
                             (2 * B <= cus * max(per_cu, 1) or large_b))
        # one-launch step: the virtual branch rides as B more workgroups of the same launch when they land on idle
        # CUs (same condition as `defer`); a batch that fills the chip by itself keeps the launch pair (its virtual
        # branch shares the local workgroups there)
        can = bool(_hip.lib().hscn_resident_train_step_supported(F, H, L, C, meta.max_n, meta.max_ell,
                                                                 meta.max_v if model.compute_virtual else 0,
                                                                 meta.max_evv if model.compute_virtual else 0))
        can = can and (self.idle_cus or not model.compute_virtual or V == 0)
        if one_launch is None:
            one_launch = can and os.environ.get("HSCN_ONE_LAUNCH", "1") != "0"
        elif one_launch and not can:
            raise RuntimeError("the one-launch step does not take this batch / model (H in {16, 32}, graphs that fit "
                               "its LDS layout, virtual branch on idle CUs only)")
        self.one_launch = bool(one_launch)
        if structure == "batch":
            structure = getattr(batch, "structure", None)
            if structure is None:
                raise ValueError("the batch carries no structure (engine.build_structure(batch) attaches one)")
        if structure is not None and not self.one_launch:
            raise RuntimeError("dataset-resident structure is a mode of the one-launch step")
        self.structure = structure
        self._sync = torch.zeros(32 + B, dtype=torch.int32, device=dev) if self.one_launch else None
        P = int(_hip.lib().hscn_resident_param_count(F, H, L, C))
        self.P = P
        self.partials = torch.empty(B, P + 1, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(P + 1, dtype=torch.float32, device=dev)
        self.loss = self.grads[P:P + 1].view(())
        if self.class_index:
            from .loss import softmax_nll_workspace
            f32 = dict(dtype=torch.float32, device=dev)
            self.score = torch.empty(B, C, **f32)                 # log-probabilities
            self.g_pred = torch.empty(B, C, **f32)
            self._loss1 = torch.zeros(1, **f32)
            self.loss = self._loss1.view(())
            self.class_flags = torch.zeros(1, dtype=torch.int32, device=dev)
            self._nll_ws = softmax_nll_workspace(B, C, dev)
            self._tail = None
        else:
            self._tail = _engine._LossTail(ptr(self.pred), ptr(self.target), int(self.kind))
        # parameter -> slice of the flat gradient buffer (launch order: {W_ll, b_ll} per layer, W1, b1, W2, b2)
        mp = model._resident_params()
        order = [p for l in range(L) for p in mp[9 * l: 9 * l + 2]] + list(mp[9 * L:])
        self.param_grads = list(zip(order, _engine.grad_views(self.grads, [p.shape for p in order], P)))

    def _job(self, xv_out: Optional[Tensor]) -> "_engine._VirtualJob":
        return _engine.virtual_job(self.x_virtual, self.ei[VV], self.ei[LV], self.meta, self._table, self.slope,
                                   self._state, xv_out)

    @property
    def advances_sync(self) -> bool:
        """Every ``run()`` adds one to word 0 of ``_sync`` on the device (the one-launch step with the virtual branch
        on its own workgroups does: its gradient fold advances the hand-off epoch) -- a per-step counter that a
        captured batch gather can read its slice number from (``DeviceHeteroDataset.gather_next(step)``)."""
        return bool(self.one_launch and self.idle_cus and self.virtual is not None and self.dims[4] >= 2
                    and self._sync is not None)

    def run(self) -> Tensor:
        """Issue the step on the current stream; returns ``loss`` (valid once the stream has run)."""
        m = self.meta
        ei_ll = self.ei[LL]
        if self.one_launch:
            N, V, F, H, L, C, B = self.dims
            W1, b1, W2, b2 = self._head
            with_v = self.idle_cus and self.virtual is not None
            call("hscn_resident_train_step", ptr(self.x_local), ptr(ei_ll), ei_ll.size(1),
                 ptr(m.lptr), ptr(m.eptr_ll), N, B, F, H, L, C, self.head_act, self._table, ptr(W1), ptr(b1), ptr(W2),
                 ptr(b2), m.max_n, m.max_ell, ptr(self.target), int(self.kind), ptr(self.pred), ptr(self.score),
                 ptr(self.partials), ptr(self.grads), ptr(self.acts) if with_v else None,
                 ptr(self._sync) if with_v else None, ptr(m.flag),
                 ctypes.byref(self._job(self.virtual)) if with_v else None,
                 ctypes.byref(self.structure.c) if self.structure is not None else None, self._grad_flags, stream())
            return self.loss
        if self.defer:
            _engine.launch_fwd_with_virtual(self._store, self.x_local, ei_ll, m, self.dims, self.head_act, self._table,
                                            self._head, self._out, self._job(None))
        else:
            _engine.launch_fwd(self._store, self.x_local, self.x_virtual, ei_ll, self.ei[VV], self.ei[LV], m, self.dims,
                               self.head_act, self.slope, self._table, self._head, self.model.compute_virtual,
                               self._out, self.virtual)
        g_pred = None
        if self.class_index:
            from .loss import launch_softmax_nll
            launch_softmax_nll(self.pred, self.target, self._loss1, self.score, self.g_pred, self.class_flags,
                               self._nll_ws)
            g_pred = self.g_pred
        _engine.launch_bwd(self._grad_flags, self.x_local, ei_ll, m, self.dims, self.head_act, self._wll_table,
                           self._head[0], self._head[2], self.acts, self.pooled, self.z, self.csr, g_pred, None,
                           self.partials, self.grads, self._tail, self._job(self.virtual) if self.defer else None)
        return self.loss

    def check(self) -> None:
        """Synchronising validity check of the launches issued so far (block-diagonal batch, sizes; with class-index
        targets also their range: ``IndexError``, the flag word is cleared)."""
        self.meta.check()
        if self.class_index:
            from .loss import raise_for_class_flags
            f = int(self.class_flags.item())
            if f:
                self.class_flags.zero_()
            raise_for_class_flags(f)


class ScnWorkspace:
    """Output / scratch buffers of the stage-A launches sized for the largest step of a loop, shared by all of its
    ``ScnTrainStep`` objects (a step uses a prefix): one set of gradient buffers means one captured optimizer step
    serves every graph of the reference's one-optimizer-step-per-graph loop (train/train_clustering.py:36-50)."""

    def __init__(self, device, max_nodes: int, max_edges: int, max_graphs: int, F: int, H: int, K: int,
                 dtype=torch.float32):
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        N, E, B = max(int(max_nodes), 1), max(int(max_edges), 1), max(int(max_graphs), 1)
        self.cap = (N, E, B)
        self.S = torch.empty(N, K, **f32)
        self.y = torch.empty(N, H, dtype=dtype, device=device)
        self.stats = torch.empty(B, 4, **f32)
        self.ss = torch.empty(B, K, K, **f32)
        self.losses = torch.empty(3, **f32)
        self.ex = (torch.empty(N + B, **i32), torch.empty(E, **i32), torch.empty(N + B, **i32), torch.empty(E, **i32),
                   torch.empty(N, 16, **f32), torch.empty(N, **f32))
        P = int(_hip.lib().hscn_scn_resident_param_count(F, H, K))
        self.partials = torch.empty(B, P, **f32)
        self.grads = torch.zeros(P, **f32)
        self.one = torch.ones(1, **f32)
        self.ticket = torch.zeros(1, **i32)
        self.flag = torch.zeros(1, **i32)


class _ScnStructC(ctypes.Structure):      # include/hscn.h: hscn_scn_structure
    _fields_ = [("rowptr_d", ctypes.c_void_p), ("col_d", ctypes.c_void_p), ("rowptr_s", ctypes.c_void_p),
                ("col_s", ctypes.c_void_p), ("agg", ctypes.c_void_p), ("dout", ctypes.c_void_p), ("xpad", ctypes.c_void_p),
                ("ready", ctypes.c_int)]


class ScnStructurePool:
    """HBM for the per-batch structure (``hscn_scn_structure``) of every step of a stage-A loop, allocated once:
    ``take(N, E, B)`` hands a step its slices.  What it holds is derived from the graphs and the input features
    alone, so a step builds it on its first visit and loads it on the others (train/train_clustering.py:34 revisits
    every graph ``cluster_epochs`` times)."""

    def __init__(self, device, total_nodes: int, total_edges: int, total_graphs: int):
        i32 = dict(dtype=torch.int32, device=device)
        self._rp = [torch.empty(max(total_nodes + total_graphs, 1), **i32) for _ in range(2)]
        self._col = [torch.empty(max(total_edges, 1), **i32) for _ in range(2)]
        # (node-indexed arrays are sliced at the row-pointer offsets, which count one more word per graph)
        self._agg = torch.empty(max(total_nodes + total_graphs, 1), 16, dtype=torch.float32, device=device)
        self._dout = torch.empty(max(total_nodes + total_graphs, 1), dtype=torch.float32, device=device)
        self._xpad = torch.empty(max(total_nodes + total_graphs, 1), 16, dtype=torch.float32, device=device)
        self._n = self._e = 0

    def take(self, N: int, E: int, B: int) -> _ScnStructC:
        n, e = self._n, self._e
        if n + N + B > self._rp[0].numel() or e + E > self._col[0].numel():
            raise ValueError("the structure pool is smaller than the loop's graphs")
        self._n, self._e = n + N + B, e + E
        p = _hip.ptr
        return _ScnStructC(p(self._rp[0][n:]), p(self._col[0][e:]), p(self._rp[1][n:]), p(self._col[1][e:]),
                           p(self._agg[n:]), p(self._dout[n:]), p(self._xpad[n:]), 0)


class ScnTrainStep:
    """``optimizer.zero_grad(); S, mc, o = model.forward_graphs(data); (mc + o).backward()`` -- the body of
    the reference's clustering loop (train/train_clustering.py:37-49) for one ``Data`` graph or a block-diagonal
    ``Batch`` of raw graphs -- as the two graph-resident launches on preallocated buffers.

    Outputs refreshed by ``run()``: ``S`` [N,K] (softmax assignment), ``losses`` [3] = {mincut, ortho, their sum},
    ``grads`` (flat: W_rel, b_rel, W_root, W_mlp, b_mlp)."""

    def __init__(self, model, data, workspace: Optional[ScnWorkspace] = None, one_launch: Optional[bool] = None,
                 structure_pool: Optional["ScnStructurePool"] = None):
        """``one_launch``: forward, losses and backward of a graph in ONE workgroup program
        (``hscn_scn_resident_train_step``).  Default: whenever the graphs fit; ``False`` keeps the forward /
        backward pair.  ``structure_pool``: keep this batch's CSRs, out-degrees and ``A_hat x`` in HBM after the first
        ``run()`` and load them on later visits (one-launch step only; same results bit for bit)."""
        from .model.hscn import SCN
        if not isinstance(model, SCN):
            raise TypeError("ScnTrainStep drives graph_hscn.model.hscn.SCN")
        if not model.resident_ok(data):
            raise RuntimeError("the fused stage-A step needs the reference's SCN shape (mp_units=[H], mlp_units=[]) "
                               "and graphs that fit one CU's LDS")
        conv, lin = model.mp.module_0, list(model.mlp)[0]
        dev = conv.lin_rel.weight.device
        self.model = model
        self.meta = meta = _engine.scn_meta(data, dev)
        x = data.x if data.x.is_cuda else data.x.to(dev)
        self.x = (x if x.dtype == torch.float16 else x.float()).contiguous()
        self._store = _engine.storage_flag(self.x.dtype)
        self.ei = (data.edge_index if data.edge_index.is_cuda else data.edge_index.to(dev)).contiguous()
        self.act = _engine.ACT[model.mp.act]
        self._mp = [conv.lin_rel.weight, conv.lin_rel.bias, conv.lin_root.weight, lin.weight, lin.bias]
        N, F = self.x.shape
        H, K = conv.lin_rel.weight.shape[0], lin.weight.shape[0]
        B, E = meta.num_graphs, self.ei.size(1)
        self.dims = (N, F, H, K, B, E)
        fits = bool(_hip.lib().hscn_scn_resident_train_step_supported(F, H, K, meta.max_n, meta.max_e))
        if one_launch and not fits:
            raise RuntimeError("one_launch=True: a graph of this batch does not fit the one-launch stage-A step")
        self.one_launch = fits if one_launch is None else bool(one_launch)
        ws = workspace if workspace is not None else ScnWorkspace(dev, N, E, B, F, H, K, self.x.dtype)
        if N > ws.cap[0] or E > ws.cap[1] or B > ws.cap[2] or ws.y.dtype != self.x.dtype:
            raise ValueError("the shared workspace is smaller than this step (or of another storage type)")
        self.workspace = ws
        if workspace is not None:        # the loop's steps share one ticket / flag word as well
            meta.ticket, meta.flag = ws.ticket, ws.flag
        elif meta.ticket is None:
            meta.ticket = ws.ticket
        self.S, self.y, self.stats, self.ss = ws.S[:N], ws.y[:N], ws.stats[:B], ws.ss[:B]
        self.losses, self.ex, self.partials, self.grads, self.one = ws.losses, ws.ex, ws.partials, ws.grads, ws.one
        self.param_grads = list(zip(self._mp, _engine.grad_views(self.grads, [p.shape for p in self._mp],
                                                                  self.grads.numel())))
        self._one_args = {}
        self._cache = structure_pool.take(N, E, B) if (structure_pool is not None and self.one_launch) else None
        self._pool = structure_pool        # ``_cache`` holds raw device pointers into the pool's buffers: keep them alive

    @property
    def loss(self) -> Tensor:
        return self.losses[2]

    def bind_grads(self) -> None:
        for p, g in self.param_grads:
            p.grad = g

    def fuses_optimizer(self, opt) -> bool:
        """``run(opt=opt)`` can apply ``opt`` (an ``optim.FlatAdam`` over THIS step's ``param_grads``) inside the
        step's own launch: one graph per step, the one-launch kernel, parameters that are their own storage."""
        return (self.one_launch and self.dims[4] == 1 and opt is not None and getattr(opt, "grads", None) is self.grads
                and all(p.is_contiguous() for p in self._mp)
                and [id(p) for p in getattr(opt, "params", [])] == [id(p) for p in self._mp])

    def _one_launch_args(self, W, opt) -> tuple:
        """hscn_scn_resident_train_step's arguments up to ``flags`` (``W``: the five parameters, contiguous)."""
        N, F, H, K, B, E = self.dims
        m = self.meta
        return (ptr(self.x), ptr(self.ei) if E else None, E, ptr(m.nptr), ptr(m.eptr), N, B, F, H, K, self.act,
                *[ptr(w) for w in W], ptr(self.one), ptr(self.one), m.max_n, m.max_e, ptr(self.S), ptr(self.stats),
                ptr(self.losses), ptr(m.ticket), ptr(self.partials), ptr(self.grads), ptr(m.flag),
                ctypes.byref(opt.c) if opt is not None else None,
                ctypes.byref(self._cache) if self._cache is not None else None)

    def run(self, opt=None) -> Tensor:
        """``opt``: ``optimizer.step()`` (train/train_clustering.py:50) in the tail of the same launch -- see
        ``fuses_optimizer``; the parameters are updated in place, ``grads`` still receives the gradient."""
        if not self.one_launch:
            if opt is not None:
                raise ValueError("this step cannot carry the optimizer step (see ScnTrainStep.fuses_optimizer)")
            W = [p.contiguous() for p in self._mp]
            _engine.launch_scn_fwd(self._store, self.x, self.ei, self.meta, self.dims, self.act, W, self.S, self.y,
                                   self.stats, self.ss, self.losses, self.meta.ticket, self.ex)
            _engine.launch_scn_bwd(self._store, self.x, self.ei, self.meta, self.dims, self.act, W[3], self.S, self.y,
                                   self.stats, self.ss, self.one, self.one, self.ex, self.partials, self.grads)
            return self.losses[2]
        # the argument list of a step is the same every visit (device pointers of buffers allocated once, the
        # parameters' own storage): built on the first call, per optimizer; a visit is then ONE foreign call
        key = id(opt)
        hit = self._one_args.get(key)
        if hit is None or hit[0] != tuple(p.data_ptr() for p in self._mp):
            if opt is not None and not self.fuses_optimizer(opt):
                raise ValueError("this step cannot carry the optimizer step (see ScnTrainStep.fuses_optimizer)")
            if all(p.is_contiguous() for p in self._mp):
                hit = self._one_args[key] = (tuple(p.data_ptr() for p in self._mp), self._one_launch_args(self._mp, opt))
            else:                   # (non-contiguous parameters: copies, every call; opt is None, see fuses_optimizer)
                W = [p.contiguous() for p in self._mp]
                hit = (None, self._one_launch_args(W, None))
        call("hscn_scn_resident_train_step", *hit[1], self._store, stream())
        if self._cache is not None:
            self._cache.ready = 1          # (read at issue time: the launch in flight saw 0 and exports)
        return self.losses[2]

    def run_forward(self) -> Tensor:
        """The forward launch alone (the assignment pass, train/train_clustering.py:57-69): refreshes ``S``."""
        _engine.launch_scn_fwd(self._store, self.x, self.ei, self.meta, self.dims, self.act,
                               [p.contiguous() for p in self._mp], self.S, self.y, self.stats, self.ss, self.losses,
                               self.meta.ticket)
        return self.S

    def check(self) -> None:
        self.meta.check()


class ScnEpochRunner:
    """The reference's stage-A loop (train/train_clustering.py:34-69: one optimizer step per graph, graph after
    graph, ``cluster_epochs`` times, then the assignment pass) driven from ONE foreign call
    (``hscn_scn_resident_train_epoch``): the dataset lies in HBM as one block-diagonal ``Batch``, ONE forward launch
    over it builds every graph's CSRs / out-degrees / ``A_hat x`` (``hscn_scn_structure``), the library then issues
    one launch per graph visit (step + optimizer in its tail, structure loaded) back to back, and ONE more forward
    launch over the dataset is the assignment pass.  The arithmetic of ``ScnTrainStep.run(opt=...)`` per graph, bit
    for bit; no per-graph Python objects, uploads or calls.

    ``eligible(...)`` says whether a model / dataset / optimizer qualifies (Adam or AdamW, the one-launch step's
    shapes)."""

    @staticmethod
    def eligible(model, big, optim_type: str) -> bool:
        from .model.hscn import SCN
        if not isinstance(model, SCN) or optim_type not in ("adam", "adamW") or not model.resident_ok(big):
            return False
        conv, lin = model.mp.module_0, list(model.mlp)[0]
        H, F = conv.lin_rel.weight.shape
        K = lin.weight.shape[0]
        meta = _engine.scn_meta(big, conv.lin_rel.weight.device)
        return bool(_hip.lib().hscn_scn_resident_train_step_supported(F, H, K, meta.max_n, meta.max_e))

    def __init__(self, model, big, optim_type: str, lr: float, weight_decay: float):
        from .optim import FlatAdam
        conv, lin = model.mp.module_0, list(model.mlp)[0]
        dev = conv.lin_rel.weight.device
        self.model = model
        self.meta = meta = _engine.scn_meta(big, dev)
        x = big.x if big.x.is_cuda else big.x.to(dev)
        self.x = (x if x.dtype == torch.float16 else x.float()).contiguous()
        self._store = _engine.storage_flag(self.x.dtype)
        self.ei = (big.edge_index if big.edge_index.is_cuda else big.edge_index.to(dev)).contiguous()
        self.act = _engine.ACT[model.mp.act]
        self._mp = [conv.lin_rel.weight, conv.lin_rel.bias, conv.lin_root.weight, lin.weight, lin.bias]
        if not all(p.is_contiguous() for p in self._mp):
            raise ValueError("the epoch kernel updates the parameters in their own storage: they must be contiguous")
        N, F = self.x.shape
        H, K = conv.lin_rel.weight.shape[0], lin.weight.shape[0]
        G, E = meta.num_graphs, self.ei.size(1)
        self.dims = (N, F, H, K, G, E)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.S = torch.empty(N, K, **f32)
        self._y = torch.empty(N, H, dtype=self.x.dtype, device=dev)
        self._stats = torch.empty(G, 4, **f32)
        self._ss = torch.empty(G, K, K, **f32)
        self.losses = torch.zeros(3, **f32)
        self._ticket = torch.zeros(1, **i32)
        self._one = torch.ones(1, **f32)
        self._cache_t = (torch.empty(N + G, **i32), torch.empty(max(E, 1), **i32), torch.empty(N + G, **i32),
                         torch.empty(max(E, 1), **i32), torch.empty(max(N, 1), 16, **f32), torch.empty(max(N, 1), **f32))
        P = int(_hip.lib().hscn_scn_resident_param_count(F, H, K))
        self.grads = torch.zeros(P, **f32)
        self.param_grads = list(zip(self._mp, _engine.grad_views(self.grads, [p_.shape for p_ in self._mp], P)))
        self.optimizer = FlatAdam.from_config(optim_type, self.param_grads, self.grads, lr, weight_decay)
        self._forward(export=True)                      # one launch: every graph's structure
        c = self._cache_t
        self._xpad = torch.zeros(max(N, 1), 16, **f32)  # the features as LDS holds them: float, 16 columns
        self._xpad[:N, :F] = self.x.float()
        self._cache = _ScnStructC(ptr(c[0]), ptr(c[1]), ptr(c[2]), ptr(c[3]), ptr(c[4]), ptr(c[5]), ptr(self._xpad), 1)

    def _forward(self, export: bool) -> None:
        _engine.launch_scn_fwd(self._store, self.x, self.ei, self.meta, self.dims, self.act, self._mp, self.S, self._y,
                               self._stats, self._ss, self.losses, self._ticket, self._cache_t if export else None)

    def run(self, visits: int) -> None:
        """``visits`` graph visits in dataset order (visit v takes graph v mod G).  One call; the launches are
        asynchronous."""
        N, F, H, K, G, E = self.dims
        m = self.meta
        call("hscn_scn_resident_train_epoch", ptr(self.x), ptr(m.nptr), ptr(m.eptr), N, G, int(visits), F, H,
             K, self.act, *[ptr(p_) for p_ in self._mp], ptr(self._one), ptr(self._one), m.max_n, m.max_e,
             ctypes.byref(self._cache),
             ctypes.byref(self.optimizer.c), ptr(self.grads), ptr(self._stats), ptr(self.losses), ptr(self._ticket),
             ptr(m.flag), self._store, stream())

    def assign(self) -> Tensor:
        """The assignment pass (train/train_clustering.py:57-69) as ONE forward launch over the dataset: the soft
        assignments ``S`` [N, K] of all graphs with the weights as they are now."""
        self._forward(export=False)
        return self.S

    def check(self) -> None:
        self.meta.check()
        self.optimizer.check()


def _mpnn_default_seed0() -> int:
    """``MPNN.dropout_seed = None``: one seed derived from ``torch.initial_seed()`` (as nn.functional.dropout derives
    its default), taken once per step object; the device step counter moves it on from there."""
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF


class MPNNResidentTrainStep(_FlatGradStep):
    """``for p: p.grad = None; pred = model(batch); loss, score = criterion(loss_fn, pred, batch.y); loss.backward()``
    for the MPNN baseline (model/mpnn.py with GCNConv) as ONE launch plus the gradient fold (include/hscn.h:
    hscn_mpnn_train_step), on buffers allocated once -- ``ResidentTrainStep``'s outward contract.

    Outputs refreshed by ``run()``: ``pred`` [B,C], ``score`` [B,C] (sigmoid), ``loss`` (0-dim), ``grads`` (flat, the
    parameter gradients in ``model.parameters()`` order, then the loss).  ``bind_grads()`` points every ``p.grad`` at
    its slice.  ``accumulate``: the fold ADDS to ``grads`` (HSCN_GRAD_ACCUMULATE); ``loss`` is the last run's.

    Dropout (``model.training`` and ``model.dropout > 0``): hidden layer i of the t-th ``run()`` (t = ``step_word``,
    a device counter the fold advances) draws the mask nn.functional.dropout draws with seed ``seed0 + (L-1) t + i``;
    ``seed0`` = ``model.dropout_seed``, or derived once from ``torch.initial_seed()`` when that is None.  A captured
    step therefore draws new masks on every replay.

    The batch may be a static fixed-capacity batch: tensor shapes are capacities then, the kernel reads the real
    per-graph ranges from ``ptr32`` / ``eptr32``."""

    def __init__(self, model, batch, loss_fn: str, target: Optional[Tensor] = None, accumulate: bool = False,
                 seed0: Optional[int] = None, step_word: Optional[Tensor] = None):
        from .model.mpnn import MPNN
        from .train import batching
        batching.refuse_layered_only(model, "the one-launch MPNN step")
        if not isinstance(model, MPNN):
            raise TypeError("MPNNResidentTrainStep drives graph_hscn.model.mpnn.MPNN")
        reason = model.resident_reason(batch)
        if reason is not None:
            raise RuntimeError(f"the one-launch MPNN step does not take this model / batch: {reason}")
        dev = batch.x.device
        self.model, self.batch, self.loss_fn = model, batch, loss_fn
        F, H, C = model.resident_dims()
        L = model.num_layers
        self.x = batch.x.contiguous()
        self.ei = batch.edge_index.contiguous()
        self.ptr32 = batch.ptr32 if batch.ptr32.device == dev else batch.ptr32.to(dev)
        self.eptr32 = batch.eptr32 if batch.eptr32.device == dev else batch.eptr32.to(dev)
        self.max_n, self.max_e = int(batch.max_nodes), int(batch.max_edges)
        B = int(batch.num_graphs)
        N = int(self.x.size(0))
        self.dims = (N, F, H, L, C, B)
        y = target if target is not None else batch.y
        if y.dtype != torch.float32 or not y.is_contiguous() or y.device != dev:
            raise TypeError("targets must be a contiguous float32 tensor on the batch's device")
        self.kind = _loss_kind(loss_fn, (B, C), y)
        self.target = y
        self.act = _hip.ACT[model.activation.hscn_name]
        self.accumulate = bool(accumulate)
        self._params = [p.contiguous() for p in model.resident_params()]
        self._table = _engine._ptr_table(self._params)
        self.p = float(model.dropout) if (model.training and model.dropout > 0) else 0.0
        if seed0 is None:
            seed0 = model.dropout_seed if model.dropout_seed is not None else _mpnn_default_seed0()
        self.seed0 = int(seed0) & 0xFFFFFFFFFFFFFFFF
        f32 = dict(dtype=torch.float32, device=dev)
        self.pred = torch.empty(B, C, **f32)
        self.score = torch.empty(B, C, **f32)
        P = int(_hip.lib().hscn_mpnn_param_count(F, H, L, C))
        self.P = P
        self.partials = torch.empty(B, P + 1, **f32)
        self.grads = torch.zeros(P + 1, **f32)
        self.loss = self.grads[P:P + 1].view(())
        # the step counter (uint32 on the device; shared with whoever else reads it, e.g. a captured batch gather)
        self.step_word = step_word if step_word is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.inv_count = 1.0 / float(B * C)
        mparams = model.resident_params()
        self.param_grads = list(zip(mparams, _engine.grad_views(self.grads, [p.shape for p in mparams], P)))

    @property
    def advances_sync(self) -> bool:
        """Every ``run()`` adds one to ``step_word`` on the device."""
        return True

    def run(self) -> Tensor:
        """Issue the step on the current stream; returns ``loss`` (valid once the stream has run)."""
        N, F, H, L, C, B = self.dims
        call("hscn_mpnn_train_step", ptr(self.x), ptr(self.ei), self.ei.size(1),
             ptr(self.ptr32), ptr(self.eptr32), N, B, F, H, L, C, self.act, self._table, self.max_n, self.max_e,
             ptr(self.target), int(self.kind), self.inv_count, ptr(self.pred), ptr(self.score), ptr(self.partials),
             ptr(self.grads), ptr(self.step_word), self.p, self.seed0, ptr(self.flag),
             _hip.GRAD_ACCUMULATE if self.accumulate else 0, stream())
        return self.loss

    def check(self) -> None:
        """Synchronising validity check of the launches issued so far."""
        f = int(self.flag.item())
        if f:
            raise RuntimeError(f"the one-launch MPNN step flagged its batch (code {f}: 1 = an edge with an end outside "
                               "its graph, 2 = a graph beyond the batch's node / edge maxima)")


class VLResidentTrainStep(_FlatGradStep):
    """``for p: p.grad = None; pred = model(x_dict, edge_index_dict, batch); loss, score = criterion(loss_fn, pred,
    batch["local"].y); loss.backward()`` for ``HSCN(vl_conv="GAT")`` -- the model whose virtual branch reaches the
    prediction through the ("virtual", "to", "local") relation -- as ONE launch plus the gradient fold (include/hscn.h:
    hscn_vl_train_step), on buffers allocated once: ``MPNNResidentTrainStep``'s outward contract.

    Outputs refreshed by ``run()``: ``pred`` [B,C], ``score`` [B,C] (sigmoid), ``loss`` (0-dim), ``grads`` (flat: the
    gradients of ``model.vl_grad_order()`` in that order, then the loss).  ``param_grads`` covers exactly the parameters
    autograd gives a gradient: vl's ``lin_dst`` / ``att_src`` / ``att_dst`` are in it (exact zeros), the last layer's
    lv and vv convolutions are not (their columns of ``grads`` are zeros; ``bind_grads()`` leaves their ``.grad`` at
    None).  ``accumulate``: the fold ADDS to ``grads``; ``loss`` is the last run's.

    The batch may be a static fixed-capacity batch: tensor shapes are capacities then, the kernel reads the real
    per-graph ranges from the segment tables."""

    def __init__(self, model, batch, loss_fn: str, target: Optional[Tensor] = None, accumulate: bool = False):
        from .model.hscn import HSCN, _act_name
        if not isinstance(model, HSCN):
            raise TypeError("VLResidentTrainStep drives graph_hscn.model.hscn.HSCN")
        x_dict, ei_dict = batch.x_dict, batch.edge_index_dict
        reason = model.resident_reason(batch, x_dict)
        if reason is not None:
            raise RuntimeError(f"the one-launch vl step does not take this model / batch: {reason}")
        dev = x_dict["local"].device
        self.model, self.batch, self.loss_fn = model, batch, loss_fn
        self.meta = meta = _engine.meta_from_batch(batch, dev)
        self.x_local = x_dict["local"].contiguous()
        self.x_virtual = x_dict["virtual"].contiguous()
        self.ei = [ei_dict[k].contiguous() for k in (LL, VV, LV)]
        mparams = model.vl_params()
        L = len(model.convs)
        H, C = model.lin_1.out_channels, model.lin_2.out_channels
        N, F = self.x_local.shape
        V, B = int(self.x_virtual.shape[0]), meta.num_graphs
        self.dims = (N, V, F, H, L, C, B)
        y = target if target is not None else batch["local"].y
        if y.dtype != torch.float32 or not y.is_contiguous() or y.device != dev:
            raise TypeError("targets must be a contiguous float32 tensor on the batch's device")
        self.kind = _loss_kind(loss_fn, (B, C), y)
        self.target = y
        self.head_act = _engine.ACT[_act_name(model.activation)]
        self.slope = float(model.convs[0].convs["__".join(LV)].negative_slope)
        self.accumulate = bool(accumulate)
        self._params = [p.contiguous() for p in mparams]
        self._table = _engine._ptr_table(self._params[:14 * L])
        f32 = dict(dtype=torch.float32, device=dev)
        self.pred = torch.empty(B, C, **f32)
        self.score = torch.empty(B, C, **f32)
        P = int(_hip.lib().hscn_vl_param_count(F, H, L, C))
        self.P = P
        self.partials = torch.empty(B, P + 1, **f32)
        self.grads = torch.zeros(P + 1, **f32)
        self.loss = self.grads[P:P + 1].view(())
        # the local activations x_1 .. x_{L-1} the backward reads again
        self.workspace = torch.empty(max((L - 1) * N * H, 1), **f32)
        self.inv_count = 1.0 / float(B * C)
        dead = {id(p) for p in model.vl_dead_params()}
        order = model.vl_grad_order()
        views = _engine.grad_views(self.grads, [p.shape for p in order], P)
        self.param_grads = [(p, g) for p, g in zip(order, views) if id(p) not in dead]

    @property
    def flag(self) -> Tensor:
        return self.meta.flag

    def run(self) -> Tensor:
        """Issue the step on the current stream; returns ``loss`` (valid once the stream has run)."""
        N, V, F, H, L, C, B = self.dims
        m, ei = self.meta, self.ei
        call("hscn_vl_train_step", ptr(self.x_local), ptr(self.x_virtual), ptr(ei[0]), ei[0].size(1), ptr(ei[1]),
             ei[1].size(1), ptr(ei[2]), ei[2].size(1), ptr(m.lptr), ptr(m.vptr), ptr(m.eptr_ll), ptr(m.eptr_vv),
             ptr(m.eptr_lv), N, V, B, F, H, L, C, self.head_act, self.slope, self._table,
             *[ptr(p) for p in self._params[14 * L:]], m.max_n, m.max_v, m.max_ell, m.max_evv, ptr(self.target),
             int(self.kind), self.inv_count, ptr(self.pred), ptr(self.score), ptr(self.partials), ptr(self.grads),
             ptr(self.workspace), ptr(m.flag), int(self.accumulate), stream())
        return self.loss

    def check(self) -> None:
        """Synchronising validity check of the launches issued so far."""
        f = int(self.meta.flag.item())
        if f & 2:
            raise IndexError("an edge connects nodes of different graphs: the batch is not block-diagonal")
        if f & 4:
            raise ValueError("a graph exceeds the sizes the one-launch vl step was configured for")
        if f & 16:
            raise ValueError("a local node has more than one local -> virtual edge (the virtual -> local relation "
                             "reads one cluster per node)")
