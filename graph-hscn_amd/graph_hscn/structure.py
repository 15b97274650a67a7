"""Device-side graph structure for the hot-path kernels.

PyG's MessagePassing gathers by ``edge_index[0]`` and scatters by
``edge_index[1]`` on every call (reference model/hscn.py:32,40,85-93).  The HIP
kernels instead walk a CSR keyed by the target node, built once per
``edge_index`` tensor on the device (stable: a row keeps its edges in edge
order, the order torch's CPU ``index_add_`` sums in) and cached for the layers
and steps that reuse the same tensor.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _hip


@dataclass
class CSR:
    rowptr: Tensor   # int32 [num_rows+1]
    col: Tensor      # int32 [max(E,1)]
    eid: Tensor      # int32 [max(E,1)]  original edge number of each slot
    num_rows: int
    num_cols: int
    num_edges: int
    flag: Tensor     # int32 [1]; 1 if an edge was out of range and skipped

    def check(self) -> None:
        """Synchronising validity check (out-of-range indices)."""
        if int(self.flag.item()) != 0:
            raise IndexError("edge_index holds node ids outside [0, num_nodes)")


def build_csr(key: Tensor, other: Tensor, num_rows: int, num_cols: int) -> CSR:
    """COO(int64) -> CSR(int32) through hscn_csr_build."""
    if key.dtype != torch.int64 or other.dtype != torch.int64:
        raise TypeError("edge_index must be int64")
    dev = key.device
    E = int(key.numel())
    key = key.contiguous()
    other = other.contiguous()
    rowptr = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _hip.lib()
    ws_bytes = int(L.hscn_csr_workspace_bytes(E, num_rows))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _hip.call("hscn_csr_build", _hip.ptr(key) if E else None, _hip.ptr(other) if E else None, E, num_rows,
              num_cols, _hip.ptr(rowptr), _hip.ptr(col), _hip.ptr(eid), _hip.ptr(flag), _hip.ptr(ws),
              ws_bytes, _hip.stream())
    return CSR(rowptr, col, eid, num_rows, num_cols, E, flag)


def build_csr_pair(src: Tensor, dst: Tensor, num_src: int, num_dst: int):
    """Both stable CSRs of one edge list through hscn_csr_build_pair: (keyed by target, keyed by source) --
    bit-identical to build_csr(dst, src, num_dst, num_src) and build_csr(src, dst, num_src, num_dst), 7 launches
    instead of 16."""
    if src.dtype != torch.int64 or dst.dtype != torch.int64:
        raise TypeError("edge_index must be int64")
    dev = src.device
    E = int(src.numel())
    src = src.contiguous()
    dst = dst.contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    rowptr, rowptr_t = torch.empty(num_dst + 1, **i32), torch.empty(num_src + 1, **i32)
    col, eid = torch.empty(max(E, 1), **i32), torch.empty(max(E, 1), **i32)
    col_t, eid_t = torch.empty(max(E, 1), **i32), torch.empty(max(E, 1), **i32)
    flag = torch.zeros(1, **i32)
    L = _hip.lib()
    ws_bytes = int(L.hscn_csr_pair_workspace_bytes(E, num_src, num_dst))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _hip.call("hscn_csr_build_pair", _hip.ptr(src) if E else None, _hip.ptr(dst) if E else None, E, num_src, num_dst,
              _hip.ptr(rowptr), _hip.ptr(col), _hip.ptr(eid), _hip.ptr(rowptr_t), _hip.ptr(col_t), _hip.ptr(eid_t),
              _hip.ptr(flag), _hip.ptr(ws), ws_bytes, _hip.stream())
    return (CSR(rowptr, col, eid, num_dst, num_src, E, flag), CSR(rowptr_t, col_t, eid_t, num_src, num_dst, E, flag))


class Relation:
    """One edge type ``src -> dst``: forward CSR (keyed by target), and lazily
    the transposed CSR (keyed by source), cross positions and GCN degree norm."""

    def __init__(self, edge_index: Tensor, num_src: int, num_dst: int, both: Optional[bool] = None,
                 csr: Optional[CSR] = None):
        if edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("edge_index must be [2, E]")
        self.edge_index = edge_index
        self.num_src = int(num_src)
        self.num_dst = int(num_dst)
        self.num_edges = int(edge_index.size(1))
        self._csr_t: Optional[CSR] = None
        # both = True: the caller knows a backward through the propagate is coming (it needs the source-keyed CSR): the
        # two CSRs then come out of ONE build (hscn_csr_build_pair); otherwise the source-keyed one is built on first use
        if csr is not None:        # the caller has the target-keyed CSR of this very list already (adopt_relation)
            self.csr = csr
        elif both:
            self.csr, self._csr_t = build_csr_pair(edge_index[0], edge_index[1], self.num_src, self.num_dst)
        else:
            self.csr = build_csr(edge_index[1], edge_index[0], self.num_dst, self.num_src)
        self._pos_t: Optional[Tensor] = None
        self._dinv: Optional[Tensor] = None
        self._max_in_degree: Optional[int] = None

    @property
    def csr_t(self) -> CSR:
        if self._csr_t is None:
            self._csr_t = build_csr(self.edge_index[0], self.edge_index[1], self.num_src, self.num_dst)
        return self._csr_t

    @property
    def pos_t(self) -> Tensor:
        """CSR slot of the edge stored at each transposed-CSR slot."""
        if self._pos_t is None:
            E = self.num_edges
            dev = self.edge_index.device
            inv = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            pos = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
            _hip.call("hscn_csr_cross_positions", _hip.ptr(self.csr.eid), _hip.ptr(self.csr_t.eid), E,
                      _hip.ptr(inv), _hip.ptr(pos), _hip.stream())
            self._pos_t = pos
        return self._pos_t

    @property
    def dinv(self) -> Tensor:
        """PyG gcn_norm degree term for unit weights, no self loops: in-degree^-1/2."""
        if self._dinv is None:
            d = torch.empty(max(self.num_dst, 1), dtype=torch.float32, device=self.edge_index.device)
            _hip.call("hscn_gcn_dinv", _hip.ptr(self.csr.rowptr), self.num_dst, _hip.ptr(d), _hip.stream())
            self._dinv = d
        return self._dinv

    @property
    def max_in_degree(self) -> int:
        """Longest row of the target-keyed CSR (repeated edges and loops count).  Read off ``rowptr`` once -- one
        synchronising copy, so a caller that captures launches asks before the capture -- then a host value."""
        if self._max_in_degree is None:
            rp = self.csr.rowptr
            self._max_in_degree = int((rp[1:] - rp[:-1]).max().item()) if self.num_dst > 0 else 0
        return self._max_in_degree

    def check(self) -> None:
        self.csr.check()


_CACHE: "OrderedDict[Tuple, Relation]" = OrderedDict()
_CACHE_MAX = 64


def relation_of(edge_index: Tensor, num_src: int, num_dst: int, cache: bool = True, both: bool = False) -> Relation:
    """Structure for ``edge_index``; cached per tensor (pointer, shape, version) so
    the L layers of one forward and repeated epochs over the same batch build it once.
    both: build the source-keyed CSR together with the target-keyed one (see Relation)."""
    if not cache:
        return Relation(edge_index, num_src, num_dst, both)
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device),
           int(num_src), int(num_dst))
    rel = _CACHE.get(key)
    if rel is not None and rel.edge_index is edge_index:
        _CACHE.move_to_end(key)
        return rel
    rel = Relation(edge_index, num_src, num_dst, both)
    _CACHE[key] = rel
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return rel


def adopt_relation(edge_index: Tensor, num_src: int, num_dst: int, csr: CSR) -> Relation:
    """Enter a target-keyed CSR that was built for ``edge_index`` anyway (gcn_norm builds one for the degrees) into the
    relation cache, so that the conv layer that receives this tensor next does not build it a second time."""
    rel = Relation(edge_index, num_src, num_dst, csr=csr)
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device),
           int(num_src), int(num_dst))
    _CACHE[key] = rel
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return rel


def with_self_loops(edge_index: Tensor, num_nodes: int) -> Tensor:
    """PyG ``add_remaining_self_loops`` for unit weights: existing self loops are taken out,
    one loop per node is appended after the remaining edges (so a target-keyed stable CSR ends every row
    with its loop, the order the reference's scatter-add sums in).  Index plumbing on the device."""
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(int(num_nodes), dtype=torch.int64, device=edge_index.device)
    return torch.cat([edge_index[:, keep], loops.unsqueeze(0).expand(2, -1)], 1).contiguous()


_LOOP_CACHE: "OrderedDict[Tuple, Tuple[Tensor, Relation]]" = OrderedDict()


def self_loop_relation_of(edge_index: Tensor, num_nodes: int, both: bool = False) -> Relation:
    """Relation over ``edge_index`` + self loops (what GCNConv(add_self_loops=True) normalises and
    propagates over), cached per tensor like ``relation_of``."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device), int(num_nodes))
    hit = _LOOP_CACHE.get(key)
    if hit is not None and hit[0] is edge_index:
        _LOOP_CACHE.move_to_end(key)
        return hit[1]
    rel = Relation(with_self_loops(edge_index, num_nodes), num_nodes, num_nodes, both)
    _LOOP_CACHE[key] = (edge_index, rel)
    while len(_LOOP_CACHE) > _CACHE_MAX:
        _LOOP_CACHE.popitem(last=False)
    return rel


def host_cards(cardinalities):
    """The ``card_host`` argument of the hscn_catenc_* entry points: a host array of F int32."""
    import ctypes
    return (ctypes.c_int32 * len(cardinalities))(*[int(c) for c in cardinalities])


@dataclass
class CategoryIndex:
    """The inverted index of an integer feature tensor ``idx`` [n, F] over the rows of a categorical encoder's table
    (column c owns rows off_c .. off_c + card_c - 1): slots ``rowptr[r] .. rowptr[r + 1]`` of ``item`` hold the ids
    i with ``off_c + idx[i, c] == r`` in ascending order.  What the encoder's backward sums over."""
    rowptr: Tensor   # int32 [R + 1]
    item: Tensor     # int32 [max(n F, 1)]; slots past rowptr[R] are unwritten
    flag: Tensor     # int32 [1]; non-zero if an index was outside its column and left out
    num_items: int   # n
    cardinalities: Tuple[int, ...]
    idx: Tensor      # the tensor it was built for (keeps the cache key's pointer alive)

    @property
    def num_rows(self) -> int:
        return int(sum(self.cardinalities))

    def check(self) -> None:
        """Synchronising validity check (out-of-range categories)."""
        if int(self.flag.item()) != 0:
            raise IndexError("a categorical feature holds an index outside [0, cardinality) of its column")


def build_category_index(idx: Tensor, cardinalities) -> CategoryIndex:
    """int64 [n, F] -> CategoryIndex through hscn_catenc_index_build (a stable counting sort; no host round trip)."""
    if idx.dtype != torch.int64:
        raise TypeError("categorical features must be int64")
    cards = tuple(int(c) for c in cardinalities)
    if idx.dim() != 2 or idx.size(1) != len(cards):
        raise ValueError(f"categorical features must be [n, {len(cards)}], got {tuple(idx.shape)}")
    src = idx.contiguous()
    dev = idx.device
    n, F, R = int(idx.size(0)), len(cards), sum(cards)
    rowptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
    item = torch.empty(max(n * F, 1), dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = int(_hip.lib().hscn_catenc_index_workspace_bytes(n, F, R))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _hip.call("hscn_catenc_index_build", _hip.ptr(src) if n else None, host_cards(cards), n, F, _hip.ptr(rowptr),
              _hip.ptr(item), _hip.ptr(flag), _hip.ptr(ws), ws_bytes, _hip.stream())
    return CategoryIndex(rowptr, item, flag, n, cards, idx)


_CAT_CACHE: "OrderedDict[Tuple, CategoryIndex]" = OrderedDict()


def category_index_of(idx: Tensor, cardinalities, cache: bool = True) -> CategoryIndex:
    """CategoryIndex for ``idx``; cached per tensor (pointer, shape, strides, version) as ``relation_of`` caches a
    Relation, so repeated epochs over the same batch build it once."""
    if not cache:
        return build_category_index(idx, cardinalities)
    cards = tuple(int(c) for c in cardinalities)
    key = (idx.data_ptr(), tuple(idx.shape), tuple(idx.stride()), idx._version, str(idx.device), cards)
    hit = _CAT_CACHE.get(key)
    if hit is not None and hit.idx is idx:
        _CAT_CACHE.move_to_end(key)
        return hit
    hit = build_category_index(idx, cards)
    _CAT_CACHE[key] = hit
    while len(_CAT_CACHE) > _CACHE_MAX:
        _CAT_CACHE.popitem(last=False)
    return hit


EXPH_TYPE_LOCAL = 0          # a local edge of a batch without edge features
EXPH_TYPE_EXPANDER = 1
EXPH_MAX_VIRTUAL_NODES = 4


class ExphormerStructure:
    """The union graph Exphormer's sparse attention runs over, for one batch.

    Rows: ``N' = N + B * nv`` -- the real nodes, then the virtual nodes graph-major (row ``N + g * nv + t``).
    Edges, in this order: the local edges (``add_local_edges``), the expander edges, then for node i (ascending) and
    virtual node t of its graph the edge i -> virtual at ``i * nv + t`` of one block and virtual -> i at the same place
    of the next.  ``erow`` int32 [E_union] names every edge's feature row: a value below ``num_edge_rows`` (= E_local
    when the local edges carry features, else 0) is that row of the per-edge tensor, ``num_edge_rows + tau`` is type
    tau of the table: 0 = local without features, 1 = expander, 2 + t = node -> virtual t, 2 + nv + t = virtual t ->
    node; ``num_types = 2 + 2 nv``.

    The index tensors are plain torch index arithmetic on whatever device the inputs are on (no reduction, no host
    read).  ``rel`` (both CSRs through ``hscn_csr_build_pair``) and ``type_slots`` (the type-keyed edge list the table
    gradient walks: ``hscn_catenc_index_build``, a stable counting sort, no launch of its own) need the device and are
    built on first use."""

    def __init__(self, edge_index: Tensor, batch_vec: Tensor, num_graphs: int, expander_edge_index: Optional[Tensor],
                 num_virtual_nodes: int, add_local_edges: bool = True, edge_features: bool = True):
        nv = int(num_virtual_nodes)
        if not 0 <= nv <= EXPH_MAX_VIRTUAL_NODES:
            raise ValueError(f"num_virtual_nodes must be in [0, {EXPH_MAX_VIRTUAL_NODES}], got {num_virtual_nodes}")
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise TypeError("edge_index must be an int64 [2, E] tensor")
        dev = edge_index.device
        N, B = int(batch_vec.numel()), int(num_graphs)
        i64 = dict(dtype=torch.int64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        parts, rows = [], []
        E_local = int(edge_index.size(1))
        self.num_edge_rows = E_local if (add_local_edges and edge_features) else 0
        El = self.num_edge_rows
        if add_local_edges:
            parts.append(edge_index)
            rows.append(torch.arange(E_local, **i32) if El else torch.full((E_local,), EXPH_TYPE_LOCAL, **i32))
        if expander_edge_index is not None:
            if expander_edge_index.dtype != torch.int64 or expander_edge_index.dim() != 2 or \
                    expander_edge_index.size(0) != 2 or expander_edge_index.device != dev:
                raise TypeError(f"the expander edges must be an int64 [2, E] tensor on {dev}")
            parts.append(expander_edge_index)
            rows.append(torch.full((int(expander_edge_index.size(1)),), El + EXPH_TYPE_EXPANDER, **i32))
        if nv:
            node = torch.arange(N, **i64).repeat_interleave(nv)                      # i * nv + t -> i
            t = torch.arange(nv, **i64).repeat(N)                                    #            -> t
            virt = N + batch_vec.to(torch.int64).repeat_interleave(nv) * nv + t
            parts += [torch.stack([node, virt]), torch.stack([virt, node])]
            rows += [(El + 2 + t).to(torch.int32), (El + 2 + nv + t).to(torch.int32)]
        self.num_nodes, self.num_graphs, self.num_virtual_nodes = N, B, nv
        self.num_rows = N + B * nv
        self.num_types = 2 + 2 * nv
        self.edge_index = torch.cat(parts, 1).contiguous() if parts else torch.zeros(2, 0, **i64)
        self.erow = torch.cat(rows).contiguous() if rows else torch.zeros(0, **i32)
        self.num_edges = int(self.edge_index.size(1))
        self._rel: Optional[Relation] = None
        self._type_slots = None

    @classmethod
    def from_parts(cls, edge_index: Tensor, erow: Tensor, num_nodes: int, num_graphs: int, num_virtual_nodes: int,
                   num_edge_rows: int) -> "ExphormerStructure":
        """A union graph the caller has put together: ``edge_index`` int64 [2, E] over ``num_nodes + num_graphs *
        num_virtual_nodes`` rows in any order, ``erow`` [E] as above.  Every per-edge row below ``num_edge_rows`` must
        be named by exactly one edge (the attention's backward writes each row's gradient once); this is checked here,
        with one read of the device."""
        nv = int(num_virtual_nodes)
        if not 0 <= nv <= EXPH_MAX_VIRTUAL_NODES:
            raise ValueError(f"num_virtual_nodes must be in [0, {EXPH_MAX_VIRTUAL_NODES}], got {num_virtual_nodes}")
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise TypeError("edge_index must be an int64 [2, E] tensor")
        El, T = int(num_edge_rows), 2 + 2 * nv
        if erow.dim() != 1 or erow.numel() != edge_index.size(1) or erow.is_floating_point():
            raise ValueError("erow must hold one integer per edge")
        own = erow[erow < El].to(torch.int64)
        if erow.numel() and (int(erow.min()) < 0 or int(erow.max()) >= El + T):
            raise ValueError(f"erow holds a row outside [0, {El} + {T})")
        if own.numel() != El or (El and not bool((torch.bincount(own, minlength=El) == 1).all())):
            raise ValueError(f"every per-edge feature row in [0, {El}) must be named by exactly one edge")
        self = cls.__new__(cls)
        self.num_edge_rows, self.num_nodes, self.num_graphs, self.num_virtual_nodes = El, int(num_nodes), int(num_graphs), nv
        self.num_rows, self.num_types = self.num_nodes + self.num_graphs * nv, T
        self.edge_index = edge_index.contiguous()
        self.erow = erow.to(torch.int32).contiguous()
        self.num_edges = int(edge_index.size(1))
        self._rel, self._type_slots = None, None
        return self

    @property
    def rel(self) -> Relation:
        if self._rel is None:
            self._rel = Relation(self.edge_index, self.num_rows, self.num_rows, both=True)
        return self._rel

    @property
    def type_slots(self) -> Tuple[Tensor, Tensor]:
        """(rowptr int32 [T + 1], item int32): slots ``rowptr[tau] .. rowptr[tau + 1]`` of ``item`` hold the union edge
        ids of type tau, ascending."""
        if self._type_slots is None:
            key = (self.erow.to(torch.int64) - (self.num_edge_rows - 1)).clamp_(min=0).unsqueeze(1)   # 0: a per-edge row
            idx = build_category_index(key, (self.num_types + 1,))
            self._type_slots = (idx.rowptr[1:], idx.item, idx)
        return self._type_slots[:2]

    @classmethod
    def of(cls, batch, degree: int, num_virtual_nodes: int, add_local_edges: bool = True, seed: int = 0,
           edge_features: Optional[bool] = None, graph_ids: Optional[Tensor] = None) -> "ExphormerStructure":
        """The structure of a collated ``Batch`` on the device, built once and kept on the batch object (in the dict
        that ``train.batching.to_device`` hands on by reference, beside the shortest-path buckets).  The expander is
        drawn by ``nn.functional.expander_edges`` with ``graph_ids`` (default ``arange(B)``): a reshuffled loader draws
        a new one per batch, a batch object that is reused keeps its own."""
        from .nn.functional import expander_edges
        if edge_features is None:
            edge_features = getattr(batch, "edge_attr", None) is not None
        cache = getattr(batch, "__dict__", {}).setdefault("_spd_cache", {})
        key = ("exphormer", int(degree), int(num_virtual_nodes), bool(add_local_edges), int(seed), bool(edge_features),
               None if graph_ids is None else graph_ids.data_ptr(), str(batch.ptr32.device))
        if key not in cache:
            B = int(batch.ptr32.numel()) - 1
            N = int(batch.batch.numel())
            if graph_ids is None:
                graph_ids = torch.arange(B, dtype=torch.int32, device=batch.ptr32.device)
            ex = expander_edges(batch.ptr32, degree, seed, graph_ids, max_nodes=batch.max_nodes, num_nodes=N)
            cache[key] = cls(batch.edge_index, batch.batch, B, ex, num_virtual_nodes, add_local_edges, edge_features)
        return cache[key]


def clear_cache() -> None:
    _LOOP_CACHE.clear()
    _CACHE.clear()
    _CAT_CACHE.clear()


def segments_from_batch(batch: Tensor, num_segments: Optional[int] = None) -> CSR:
    """CSR over graphs from a PyG ``batch`` vector (any order): row g lists the
    nodes of graph g.  ``num_segments=None`` reads ``batch.max()+1`` (one sync),
    as global_mean_pool does."""
    if num_segments is None:
        num_segments = int(batch.max().item()) + 1 if batch.numel() else 0
    node = torch.arange(batch.numel(), dtype=torch.int64, device=batch.device)
    return build_csr(batch, node, int(num_segments), int(batch.numel()))
