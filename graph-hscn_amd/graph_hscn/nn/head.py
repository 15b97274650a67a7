"""The per-node head of a node-level model: ``pred = lin_2(act(lin_1(x)))`` on every row of ``x`` [N, H] as one
forward launch and one backward launch plus an ordered fold (include/hscn.h: hscn_node_head_fwd / _bwd;
csrc/node_head.hip).  ``hscn_node_head_supported`` is the single source of truth for the envelope; outside it -- or
with ``route="layered"`` -- the head is the two ``Linear`` modules it wraps, through the layered operators.  The
wrapper owns no parameters: they stay the model's ``lin_1`` / ``lin_2``."""
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
