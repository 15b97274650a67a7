"""The per-node head of a node-level model: ``pred = lin_2(act(lin_1(x)))`` on every row of ``x`` [N, H] as one
forward launch and one backward launch plus an ordered fold (include/hscn.h: hscn_node_head_fwd / _bwd;
csrc/node_head.hip).  ``hscn_node_head_supported`` is the single source of truth for the envelope; outside it -- or
with ``route="layered"`` -- the head is the two ``Linear`` modules it wraps, through the layered operators.  The
wrapper owns no parameters: they stay the model's ``lin_1`` / ``lin_2``.

The pair decoder of a link-level model: ``pair_dot(z, pair_index)`` = one score ``<z[u], z[v]>`` per candidate pair, one
forward launch and one backward launch (hscn_pair_dot_fwd / _bwd; csrc/edge_head.hip).  ``hscn_pair_dot_supported`` is
the envelope and there is no other route: outside it ``pair_dot`` raises."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from .. import _hip
from .._hip import ACT, call, ptr, stream
from .functional import _c

# which route a NodeHead takes where the fused kernels apply.  The fused head becomes the default only once
# tools/bench_node_head.py has shown its median ahead of the layered route's by more than the larger spread at both
# shapes; until that run exists the default is the layered pair and ``route="fused"`` selects
# the kernels.
DEFAULT_ROUTE = "layered"


def node_head_supported(H: int, C: int) -> bool:
    return bool(_hip.lib().hscn_node_head_supported(int(H), int(C)))


def rows_per_workgroup() -> int:
    return int(_hip.lib().hscn_node_head_rows_per_workgroup())


def node_head_fwd_raw(x: Tensor, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor, act: int) -> Tensor:
    N, H = x.shape
    C = W2.shape[0]
    pred = torch.empty(N, C, dtype=torch.float32, device=x.device)
    call("hscn_node_head_fwd", ptr(x), ptr(W1), ptr(b1), ptr(W2), ptr(b2), N, H, C, act, ptr(pred), stream())
    return pred


def node_head_bwd_raw(x: Tensor, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor, g_pred: Tensor,
                      scale: Optional[Tensor], act: int, want_gx: bool = True,
                      grads: Optional[Tuple[Tensor, Tensor, Tensor, Tensor]] = None, accumulate: bool = False):
    """``(g_x, gW1, gb1, gW2, gb2)``.  ``grads``: the four parameter gradients to write -- or, with ``accumulate``, to
    add into; fresh tensors without it."""
    N, H = x.shape
    C = W2.shape[0]
    dev = x.device
    if grads is None:
        if accumulate:
            raise ValueError("accumulate needs the gradients to add into")
        grads = tuple(torch.empty_like(p) for p in (W1, b1, W2, b2))
    g_x = torch.empty(N, H, dtype=torch.float32, device=dev) if want_gx else None
    nbytes = int(_hip.lib().hscn_node_head_workspace_bytes(N, H, C))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    call("hscn_node_head_bwd", ptr(x), ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(g_pred), ptr(scale), N, H, C, act,
         ptr(g_x), *[ptr(g) for g in grads], 1 if accumulate else 0, ptr(ws), nbytes, stream())
    return (g_x,) + tuple(grads)


def _aligned(t: Tensor) -> Tensor:
    """The launches move rows as float4: a contiguous view at an odd storage offset is copied to a fresh buffer."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class NodeHeadFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor, act: int):
        x, W1, b1, W2, b2 = _aligned(_c(x)), _c(W1), _c(b1), _c(W2), _c(b2)
        ctx.act = act
        ctx.save_for_backward(x, W1, b1, W2, b2)
        return node_head_fwd_raw(x, W1, b1, W2, b2, act)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, W1, b1, W2, b2 = ctx.saved_tensors
        # a loss.LazyScaled gradient is consumed unmultiplied: the launch applies the scalar on the way in
        if hasattr(g, "grad_unscaled"):
            g_pred, scale = g.grad_unscaled, g.scale
        else:
            g_pred, scale = _c(g), None
        if x.size(0) == 0:
            return (torch.zeros_like(x),) + tuple(torch.zeros_like(p) for p in (W1, b1, W2, b2)) + (None,)
        out = node_head_bwd_raw(x, W1, b1, W2, b2, g_pred, scale, ctx.act, want_gx=ctx.needs_input_grad[0])
        return out + (None,)


class NodeHead:
    """``lin_2(act(lin_1(x)))`` per row.  ``route``: "fused" (the one-launch kernels; an error outside their
    envelope), "layered" (the two ``Linear`` modules) or None = ``DEFAULT_ROUTE`` where the kernels apply, else
    layered."""

    def __init__(self, lin_1, lin_2, act: str, route: Optional[str] = None):
        if act not in ACT:
            raise KeyError(f"unknown activation {act!r}")
        if route not in (None, "fused", "layered"):
            raise ValueError(f"route must be None, 'fused' or 'layered', not {route!r}")
        self.lin_1, self.lin_2, self.act, self.route = lin_1, lin_2, act, route
        self.last_route: Optional[str] = None

    def supported(self) -> bool:
        H, C = self.lin_1.out_channels, self.lin_2.out_channels
        return (self.lin_1.in_channels == H and self.lin_2.in_channels == H and self.lin_1.bias is not None
                and self.lin_2.bias is not None and node_head_supported(H, C))

    def __call__(self, x: Tensor) -> Tensor:
        route = self.route
        if route is None:
            route = DEFAULT_ROUTE if self.supported() else "layered"
        elif route == "fused" and not self.supported():
            raise RuntimeError(f"the fused node head takes H in {{16, 32, 64}} and 1 <= C <= 64 with biases "
                               f"(hscn_node_head_supported), not H={self.lin_1.out_channels}, "
                               f"C={self.lin_2.out_channels}")
        self.last_route = route
        if route == "layered":
            return self.lin_2(self.lin_1(x, act=self.act))
        return NodeHeadFn.apply(x, self.lin_1.weight, self.lin_1.bias, self.lin_2.weight, self.lin_2.bias,
                                ACT[self.act])


# ---- the pair decoder -------------------------------------------------------------------------------------------------

def pair_dot_supported(D: int) -> bool:
    return bool(_hip.lib().hscn_pair_dot_supported(int(D)))


def pairs_per_workgroup(D: int) -> int:
    return int(_hip.lib().hscn_pair_dot_pairs_per_workgroup(int(D)))


class PairStructure:
    """What the pair launches need of a batch's candidate pairs besides the embeddings, integers only: the pair index
    as int32 [2, P], the two stable CSRs of the pair list (keyed by source and by target: the backward's walk) and,
    with labels, the CSR of the positive pairs keyed by source (the metric's filters).  Built once per batch --
    ``PairStructure.of(store)`` caches it on the store that carries ``edge_label_index``."""

    def __init__(self, pair_index: Tensor, num_nodes: int, edge_label: Optional[Tensor] = None):
        from ..structure import build_csr, build_csr_pair
        if pair_index.dim() != 2 or pair_index.size(0) != 2 or pair_index.dtype != torch.int64:
            raise ValueError("pair_index must be an int64 [2, P] tensor")
        _hip.ptr(pair_index)                                  # (a CPU tensor: the package's no-CPU-fallback error)
        self.num_nodes, self.num_pairs = int(num_nodes), int(pair_index.size(1))
        self.index = pair_index
        self.index32 = pair_index.to(torch.int32).contiguous()
        self.by_dst = self.by_src = self.positives = None
        self.edge_label = None
        if self.num_pairs and self.num_nodes:
            self.by_dst, self.by_src = build_csr_pair(pair_index[0], pair_index[1], self.num_nodes, self.num_nodes)
        if edge_label is not None:
            self.edge_label = edge_label.to(torch.float32).contiguous()
            if self.num_pairs and self.num_nodes:
                # a pair that is not positive gets the key -1: the build skips it (and raises a flag nobody reads)
                key = torch.where(self.edge_label == 1, pair_index[0], torch.full_like(pair_index[0], -1))
                self.positives = build_csr(key, pair_index[1].contiguous(), self.num_nodes, self.num_nodes)

    @classmethod
    def of(cls, store, num_nodes: Optional[int] = None) -> "PairStructure":
        """The structure of ``store`` (a ``Batch``, or the local node store of a ``HeteroBatch``), built on first use."""
        cached = store._d.get("_pair_structure") if hasattr(store, "_d") else None
        index = store.edge_label_index
        if cached is None or cached.index is not index:
            n = int(store.num_nodes) if num_nodes is None else int(num_nodes)
            cached = cls(index, n, store.edge_label if "edge_label" in store else None)
            if hasattr(store, "_d"):
                store._d["_pair_structure"] = cached
        return cached


def pair_dot_fwd_raw(z: Tensor, index32: Tensor, flags: Tensor) -> Tensor:
    N, D = z.shape
    P = int(index32.size(1))
    score = torch.empty(P, dtype=torch.float32, device=z.device)
    call("hscn_pair_dot_fwd", ptr(z), ptr(index32), N, P, D, ptr(score), ptr(flags), stream())
    return score


def pair_dot_bwd_raw(z: Tensor, st: PairStructure, g_score: Tensor, scale: Optional[Tensor]) -> Tensor:
    N, D = z.shape
    g_z = torch.empty(N, D, dtype=torch.float32, device=z.device)
    call("hscn_pair_dot_bwd", ptr(z), ptr(st.index32), ptr(g_score), ptr(scale), ptr(st.by_src.rowptr),
         ptr(st.by_src.eid), ptr(st.by_dst.rowptr), ptr(st.by_dst.eid), N, st.num_pairs, D, ptr(g_z), stream())
    return g_z


_PAIR_FLAGS = _hip.FlagWord()
PAIR_ID_OUT_OF_RANGE = 1          # include/hscn.h: HSCN_PAIR_ID_OUT_OF_RANGE


def pair_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every ``pair_dot`` forward ORs into (a pair id outside ``[0, N)``: its
    score is 0).  ``check_pair_ids`` reads and clears it."""
    return _PAIR_FLAGS.of(device)


def check_pair_ids(device) -> None:
    """Synchronising: ``IndexError`` if a ``pair_dot`` call since the last check met a node id outside ``[0, N)``."""
    if _PAIR_FLAGS.take(device) & PAIR_ID_OUT_OF_RANGE:
        raise IndexError("edge_label_index holds node ids outside [0, num_nodes)")


class PairDotFn(Function):
    @staticmethod
    def forward(ctx, z: Tensor, structure: PairStructure):
        z = _aligned(_c(z))
        ctx.structure = structure
        ctx.save_for_backward(z)
        if structure.num_pairs == 0:                          # nothing to launch
            return torch.empty(0, dtype=torch.float32, device=z.device)
        return pair_dot_fwd_raw(z, structure.index32, pair_flags(z.device))

    @staticmethod
    def backward(ctx, g: Tensor):
        (z,) = ctx.saved_tensors
        if ctx.structure.num_pairs == 0 or z.size(0) == 0:
            return torch.zeros_like(z), None
        # a loss.LazyScaled gradient is consumed unmultiplied: the launch applies the scalar on the way in
        if hasattr(g, "grad_unscaled"):
            g_score, scale = g.grad_unscaled, g.scale
        else:
            g_score, scale = _c(g), None
        return pair_dot_bwd_raw(z, ctx.structure, g_score, scale), None


def pair_dot(z: Tensor, pair_index: Tensor, structure: Optional[PairStructure] = None) -> Tensor:
    """``score[p] = <z[pair_index[0, p]], z[pair_index[1, p]]>`` for ``z`` [N, D] float32 on the device and
    ``pair_index`` int64 [2, P].  ``structure``: the ``PairStructure`` of this very ``pair_index`` and node count (built
    here when not given; another one is a ``ValueError``).  No pairs: nothing is launched, the score is empty and the
    gradient of ``z`` zero.  A node id outside ``[0, N)`` cannot raise from a launch: its score is 0, a bit of
    ``pair_flags(device)`` is set, and ``check_pair_ids(device)`` -- which ``train.train`` calls once per epoch --
    raises the ``IndexError``."""
    if z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError("z must be a float32 [N, D] tensor")
    _hip.ptr(z if not z.is_cuda else pair_index)              # (CPU tensors: the package's no-CPU-fallback error)
    if not pair_dot_supported(z.size(1)):
        raise RuntimeError(f"the pair decoder takes an embedding width that is a multiple of 4 in [4, 64] "
                           f"(hscn_pair_dot_supported), not D={z.size(1)}")
    if structure is None:
        structure = PairStructure(pair_index, z.size(0))
    elif structure.index is not pair_index and not (structure.index.shape == pair_index.shape
                                                    and structure.index.data_ptr() == pair_index.data_ptr()):
        raise ValueError("structure was built for another pair_index")
    elif structure.num_nodes != z.size(0):
        raise ValueError(f"structure was built for {structure.num_nodes} nodes, z has {z.size(0)} rows")
    return PairDotFn.apply(z, structure)
