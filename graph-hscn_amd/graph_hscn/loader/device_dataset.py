"""A hetero dataset that lives in HBM, and batches collated on the device.

The reference hands every step a batch collated on the host (PyG ``DataLoader`` ->
``Batch.from_data_list``; loader/hetero_data.py:91-106, loader/loader.py:48-60): ~10 ms of Python for a
128-graph batch against a 47 us training step, plus a PCIe copy.  An MI355X has 288 GB: the whole Peptides
hetero dataset is ~250 MB.  ``DeviceHeteroDataset`` keeps it resident as concatenated arrays (edge lists with
per-graph LOCAL node ids, int32) and ``gather(ids)`` writes the batch made of graphs ``ids`` -- a slice of the
epoch's permutation, itself a device tensor -- into the fixed-capacity buffers of a ``StaticHeteroBatch`` with
ONE launch (``hscn_collate_gather``), bit for bit what ``HeteroBatch.from_data_list`` builds for the same list.
An epoch is then ``perm = torch.randperm(G, device=...)`` and, per step, ``ds.gather(perm[i:i+B]);
step.replay(); optimizer.step()`` with no host work that scales with the batch.

``DeviceGraphDataset`` is the same for the MPNN baseline's homogeneous graphs.  Both are a ``_DeviceDataset``: the
subclasses only lay their tables out as ``hscn_hetero_dataset`` / ``hscn_hetero_batch_out``.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch
from torch import Tensor

from .. import _hip
from ..data import HeteroBatch, HeteroData, has_link_labels
from ..replay import LL, LV, VV, StaticHeteroBatch

_RELS = (LL, VV, LV)     # include/hscn.h: relation order of hscn_hetero_dataset / hscn_hetero_batch_out


class _Dataset(ctypes.Structure):
    _fields_ = [("x_local", ctypes.c_void_p), ("x_virtual", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("nptr", ctypes.c_void_p), ("vptr", ctypes.c_void_p), ("src", ctypes.c_void_p * 3),
                ("dst", ctypes.c_void_p * 3), ("eptr", ctypes.c_void_p * 3), ("G", ctypes.c_int64),
                ("F", ctypes.c_int32), ("C", ctypes.c_int32)]


class _BatchOut(ctypes.Structure):
    _fields_ = [("x_local", ctypes.c_void_p), ("x_virtual", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("ptr_local", ctypes.c_void_p), ("ptr_virtual", ctypes.c_void_p), ("ptr32_local", ctypes.c_void_p),
                ("ptr32_virtual", ctypes.c_void_p), ("batch_local", ctypes.c_void_p), ("batch_virtual", ctypes.c_void_p),
                ("ei", ctypes.c_void_p * 3), ("eptr32", ctypes.c_void_p * 3), ("ncap", ctypes.c_int64),
                ("vcap", ctypes.c_int64), ("ecap", ctypes.c_int64 * 3)]


def _top_sum(sizes: Tensor, k: int) -> int:
    """Largest total any ``k`` graphs can have."""
    return int(torch.topk(sizes, min(k, sizes.numel())).values.sum()) if sizes.numel() else 0


class _DeviceDataset:
    """What the two datasets share: the gather launches and an epoch that walks by itself.  A subclass's constructor
    calls this one first, then fills ``F``, ``C``, ``_t`` (its device tables), ``static`` (the fixed-capacity batch the
    gathers write), ``_ds`` / ``_out`` (the two as the C structs) and, optionally, ``structure`` / ``_out_structure``
    (per-graph structure gathered with every batch)."""

    def __init__(self, graphs: Sequence, device, batch_size: int):
        if not graphs:
            raise ValueError("empty dataset")
        for g in graphs:      # (the gather launches know nothing of candidate pairs: refuse, never drop them)
            store = g["local"] if isinstance(g, HeteroData) else g
            if has_link_labels(store):
                raise ValueError(f"{type(self).__name__} does not carry link labels (edge_label_index / edge_label): "
                                 "a link-level model trains from host loaders (train.train)")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_graphs = len(graphs)
        self.batch_size = int(batch_size)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.structure = None
        self._perm: Optional[Tensor] = None
        self._cursor: Optional[Tensor] = None
        self._counters: dict = {}      # id(step) -> (the step's per-step device counter, its value at epoch start, step)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._t.values() if t is not None)

    def _gather(self, ids: Tensor, cur, base):
        """Batch ``ids[c * batch_size:(c + 1) * batch_size]`` into ``self.static``, c = ``*cur - *base`` (0 for None);
        a ``cur`` without a ``base`` is the dataset's own cursor, which the gather proper advances."""
        if self.structure is not None:        # (before the gather proper: that call advances the cursor)
            _hip.call("hscn_collate_gather_structure", ctypes.byref(self._ds), ctypes.byref(self.structure.c),
                      _hip.ptr(ids), self.batch_size, ctypes.byref(self._out), ctypes.byref(self._out_structure.c),
                      _hip.ptr(self.flag), cur, base, _hip.stream())
        _hip.call("hscn_collate_gather", ctypes.byref(self._ds), _hip.ptr(ids), self.batch_size,
                  ctypes.byref(self._out), _hip.ptr(self.flag), cur, base, _hip.stream())
        return self.static.batch

    def gather(self, ids: Tensor):
        """Make ``self.static`` hold the batch of graphs ``ids`` (int64 ``[batch_size]`` on the device; order
        kept).  Asynchronous on the current stream, capturable; returns ``self.static.batch``."""
        if ids.dtype != torch.int64 or ids.device != self.device or ids.numel() != self.batch_size:
            raise ValueError(f"ids must be int64 [{self.batch_size}] on {self.device}")
        return self._gather(ids.contiguous(), None, None)

    # ---- an epoch that walks by itself: the permutation and a batch counter live on the device ----------------
    def new_epoch(self, generator: Optional[torch.Generator] = None) -> Tensor:
        """Draw the epoch's permutation into the dataset's own buffer and rewind the batch counter.  Returns the
        permutation (a device tensor; ``gather_next`` serves its first ``num_graphs // batch_size`` slices)."""
        if self._perm is None:
            # (one spare batch of valid ids behind the permutation: a replay too many reads those, not stray memory)
            self._perm_buf = torch.zeros(self.num_graphs + self.batch_size, dtype=torch.int64, device=self.device)
            self._perm = self._perm_buf[: self.num_graphs]
            self._cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
        torch.randperm(self.num_graphs, device=self.device, generator=generator, out=self._perm)
        self._cursor.zero_()
        for counter, base, _ in self._counters.values():   # steps with a counter of their own: this epoch's slices
            base.copy_(counter)                            # count from its value now
        return self._perm

    def gather_next(self, step=None):
        """Gather the next batch of the current epoch's permutation and advance the device-side counter, with no
        host argument that changes from step to step, so the launches can be CAPTURED in front of the training step
        (``CapturedStep(..., pre=ds.gather_next)``) -- a replay is then "next batch + iteration".
        ``step``: the resident step the gather is captured with (``CapturedStep`` passes it).  When that step
        keeps a per-step counter on the device (word 0 of the one-launch step's sync buffer, advanced by its gradient
        fold), the gather reads its slice number off THAT counter (minus its value when the epoch began) and the
        launch that would advance a counter of our own (4.5 us per iteration) does not exist."""
        if self._perm is None:
            raise RuntimeError("call new_epoch() first")
        sync = getattr(step, "_sync", None) if step is not None else None
        if sync is not None and getattr(step, "advances_sync", False):
            ent = self._counters.get(id(step))
            if ent is None:                      # (uint32 counter read as int32; the base is this epoch's start)
                ent = self._counters[id(step)] = (sync[:1], sync[:1].clone(), step)
            return self._gather(self._perm, _hip.ptr(ent[0]), _hip.ptr(ent[1]))
        return self._gather(self._perm, _hip.ptr(self._cursor), None)

    def check(self) -> None:
        """Synchronising validity check of the gathers issued so far."""
        if int(self.flag.item()) & 8:
            raise IndexError("a graph id was outside the dataset (or a batch exceeded the static capacity)")


class DeviceHeteroDataset(_DeviceDataset):
    """``graphs``: the list ``generate_hetero_data`` returns (or any sequence of ``HeteroData`` with the
    local / virtual node types and the ll / vv / lv relations).  ``batch_size`` graphs per step."""

    def __init__(self, graphs: Sequence[HeteroData], device, batch_size: int, resident_structure: bool = False):
        """``resident_structure``: also keep every graph's CSRs (ll by target and by source, lv, vv; graph-local
        ids) and degree norms in HBM -- built ONCE here by ``hscn_resident_structure`` over the dataset laid out as
        one batch -- and gather them with every batch (``static.batch.structure``), so that a step can load its
        structure instead of rebuilding it (``CapturedStep(..., structure="batch")``).  +~40 % dataset bytes."""
        super().__init__(graphs, device, batch_size)
        whole = HeteroBatch.from_data_list(graphs)            # once, on the host: global ids + per-graph ranges
        nptr, vptr = whole["local"].ptr, whole["virtual"].ptr
        base = {"local": nptr, "virtual": vptr}
        self.F = int(whole["local"].x.size(1))
        y = whole["local"].y if "y" in whole["local"] else None
        # class-index targets (one integer per graph, data.py's collation of ``y = tensor([c])``): kept as int64 [G];
        # the gather copies a graph's target row as float32 WORDS, so an int64 travels as a row of two, bit for bit
        self.class_index = y is not None and y.dim() == 1 and not y.dtype.is_floating_point
        self.C = None if (y is None or self.class_index) else int(y.size(1))
        y_words = 2 if self.class_index else (self.C or 0)
        dev = self.device
        if y is not None:
            y = (y.to(torch.int64) if self.class_index else y.float()).contiguous().to(dev)
        self._t = {"x_local": whole["local"].x.float().contiguous().to(dev),
                   "x_virtual": whole["virtual"].x.float().contiguous().to(dev),
                   "y": y,
                   "nptr": nptr.to(dev), "vptr": vptr.to(dev)}
        sizes = {"local": nptr[1:] - nptr[:-1], "virtual": vptr[1:] - vptr[:-1]}
        esizes = {}
        for r, et in enumerate(_RELS):
            ei = whole[et].edge_index
            eptr = whole[et].ptr32.to(torch.int64)
            esizes[et] = eptr[1:] - eptr[:-1]
            owner = torch.repeat_interleave(torch.arange(self.num_graphs), esizes[et])
            s, _, d = et
            self._t[f"src{r}"] = (ei[0] - base[s][owner]).to(torch.int32).contiguous().to(dev)
            self._t[f"dst{r}"] = (ei[1] - base[d][owner]).to(torch.int32).contiguous().to(dev)
            self._t[f"eptr{r}"] = eptr.contiguous().to(dev)
        B = self.batch_size
        self.static = StaticHeteroBatch.from_capacities(
            B, dev, _top_sum(sizes["local"], B), _top_sum(sizes["virtual"], B),
            {et: _top_sum(esizes[et], B) for et in _RELS},
            {"local": int(sizes["local"].max()), "virtual": int(sizes["virtual"].max())},
            {et: int(esizes[et].max()) if esizes[et].numel() else 0 for et in _RELS}, self.F, self.C,
            class_index=self.class_index)
        if resident_structure:
            from ..engine import BatchStructure, build_structure
            self.structure = build_structure(whole.to(dev))              # one launch over all G graphs
            st0 = self.static
            self._out_structure = BatchStructure(dev, st0.N, st0.V, B, st0.E[LL], st0.E[LV], st0.E[VV])
            st0.batch.structure = self._out_structure
            torch.cuda.synchronize(dev)                                   # (the int64 COO copy of `whole` may go now)
        t = self._t
        p = _hip.ptr
        self._ds = _Dataset(p(t["x_local"]), p(t["x_virtual"]), p(t["y"]), p(t["nptr"]), p(t["vptr"]),
                            (ctypes.c_void_p * 3)(*[p(t[f"src{r}"]) for r in range(3)]),
                            (ctypes.c_void_p * 3)(*[p(t[f"dst{r}"]) for r in range(3)]),
                            (ctypes.c_void_p * 3)(*[p(t[f"eptr{r}"]) for r in range(3)]),
                            self.num_graphs, self.F, y_words)
        hb, st = self.static.batch, self.static
        self._out = _BatchOut(p(hb["local"].x), p(hb["virtual"].x), p(hb["local"].y) if y_words else None,
                              p(hb["local"].ptr), p(hb["virtual"].ptr), p(hb["local"].ptr32), p(hb["virtual"].ptr32),
                              p(hb["local"].batch), p(hb["virtual"].batch),
                              (ctypes.c_void_p * 3)(*[p(hb[et].edge_index) for et in _RELS]),
                              (ctypes.c_void_p * 3)(*[p(hb[et].ptr32) for et in _RELS]),
                              st.N, st.V, (ctypes.c_int64 * 3)(*[st.E[et] for et in _RELS]))


class StaticGraphBatch:
    """Fixed-capacity device buffers of a homogeneous ``Batch`` (``.batch`` is the object to hand to
    ``step.MPNNResidentTrainStep``): ``x`` [ncap, F], ``edge_index`` [2, ecap], ``batch`` [ncap], ``ptr`` / ``ptr32`` /
    ``eptr32`` [B + 1], ``y`` [B, C], and the per-graph maxima that size the kernel's LDS.  Valid inside the per-graph
    ranges of ``ptr32`` / ``eptr32`` only; the tail of every buffer is stale data of earlier, larger batches."""

    def __init__(self, B: int, device, ncap: int, ecap: int, max_nodes: int, max_edges: int, F: int, C: Optional[int]):
        from ..data import Batch
        dev = torch.device(device)
        self.device, self.num_graphs = dev, int(B)
        self.N, self.E = max(int(ncap), 1), max(int(ecap), 1)
        i64 = dict(dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        b = Batch(x=torch.zeros(self.N, F, dtype=torch.float32, device=dev),
                  edge_index=torch.zeros(2, self.E, **i64), num_nodes=self.N)
        b.y = torch.zeros(B, C, dtype=torch.float32, device=dev) if C else None
        b.batch = torch.zeros(self.N, **i64)
        b.ptr = torch.zeros(B + 1, **i64)
        b.ptr32 = torch.zeros(B + 1, **i32)
        b.eptr32 = torch.zeros(B + 1, **i32)
        b.num_graphs = int(B)
        b.max_nodes, b.max_edges = int(max_nodes), int(max_edges)
        self.batch = b
        # the (empty) virtual node type and vv / lv relations of the gather's output
        self._v = {"x": torch.zeros(1, F, dtype=torch.float32, device=dev), "batch": torch.zeros(1, **i64),
                   "ptr": torch.zeros(B + 1, **i64), "ptr32": torch.zeros(B + 1, **i32),
                   "ei": [torch.zeros(2, 1, **i64) for _ in range(2)], "eptr32": [torch.zeros(B + 1, **i32) for _ in range(2)]}


class DeviceGraphDataset(_DeviceDataset):
    """The MPNN baseline's dataset: a list of ``Data`` graphs resident in HBM, gathered into the fixed-capacity buffers
    of a ``StaticGraphBatch`` -- bit for bit what ``Batch.from_data_list`` builds (features cast to float32, as
    train/train.py:79 casts them).  It is ``hscn_collate_gather`` over a hetero dataset whose virtual node type
    has no nodes and whose vv / lv relations have no edges: every graph's virtual and vv / lv ranges are empty, so the
    blocks of those parts copy nothing and write empty segment tables."""

    def __init__(self, graphs: Sequence, device, batch_size: int):
        from ..data import Batch
        super().__init__(graphs, device, batch_size)
        G, B = self.num_graphs, self.batch_size
        whole = Batch.from_data_list(graphs)                  # once, on the host: global ids + per-graph ranges
        nptr = whole.ptr
        eptr = whole.eptr32.to(torch.int64)
        self.F = int(whole.x.size(1))
        y = getattr(whole, "y", None)
        self.C = None if y is None else int(y.size(1))
        dev = self.device
        sizes, esizes = nptr[1:] - nptr[:-1], eptr[1:] - eptr[:-1]
        owner = torch.repeat_interleave(torch.arange(G), esizes)
        ei = whole.edge_index
        zeros_g = torch.zeros(G + 1, dtype=torch.int64)
        self._t = {"x": whole.x.float().contiguous().to(dev), "xv": torch.zeros(1, self.F, device=dev),
                   "y": None if y is None else y.float().contiguous().to(dev), "nptr": nptr.to(dev),
                   "vptr": zeros_g.to(dev), "src0": (ei[0] - nptr[owner]).to(torch.int32).contiguous().to(dev),
                   "dst0": (ei[1] - nptr[owner]).to(torch.int32).contiguous().to(dev), "eptr0": eptr.contiguous().to(dev),
                   "none": torch.zeros(1, dtype=torch.int32, device=dev), "eptr_none": zeros_g.to(dev)}
        self.static = StaticGraphBatch(B, dev, _top_sum(sizes, B), _top_sum(esizes, B), int(sizes.max()),
                                       int(esizes.max()) if esizes.numel() else 0, self.F, self.C)
        t, p = self._t, _hip.ptr
        self._ds = _Dataset(p(t["x"]), p(t["xv"]), p(t["y"]), p(t["nptr"]), p(t["vptr"]),
                            (ctypes.c_void_p * 3)(p(t["src0"]), p(t["none"]), p(t["none"])),
                            (ctypes.c_void_p * 3)(p(t["dst0"]), p(t["none"]), p(t["none"])),
                            (ctypes.c_void_p * 3)(p(t["eptr0"]), p(t["eptr_none"]), p(t["eptr_none"])),
                            G, self.F, self.C or 0)
        st, b, v = self.static, self.static.batch, self.static._v
        self._out = _BatchOut(p(b.x), p(v["x"]), p(b.y) if self.C else None, p(b.ptr), p(v["ptr"]), p(b.ptr32),
                              p(v["ptr32"]), p(b.batch), p(v["batch"]),
                              (ctypes.c_void_p * 3)(p(b.edge_index), p(v["ei"][0]), p(v["ei"][1])),
                              (ctypes.c_void_p * 3)(p(b.eptr32), p(v["eptr32"][0]), p(v["eptr32"][1])),
                              st.N, 0, (ctypes.c_int64 * 3)(st.E, 1, 1))
