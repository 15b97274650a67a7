"""Operators of the hot path as autograd Functions over the HIP C ABI.

Every forward/backward here is one or more ``hscn_*`` calls (include/hscn.h) on
the current HIP stream; nothing falls back to eager PyTorch arithmetic.  The
semantics are those of the torch_geometric operators the reference calls
(model/hscn.py:6-14).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from .. import _hip
from .._hip import ACT, call, ptr, stream
from ..structure import CSR, Relation, category_index_of, host_cards


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"hot-path tensors are float32 (got {t.dtype})")
    return t.contiguous()


# --------------------------------------------------------------------------- #
# raw launchers (no autograd)
# --------------------------------------------------------------------------- #
def linear_raw(x: Tensor, W: Tensor, bias: Optional[Tensor] = None, x2: Optional[Tensor] = None,
               W2: Optional[Tensor] = None, att: Optional[Tensor] = None, act: int = 0,
               w_layout: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
    rows, in_f = x.shape
    out_f = W.shape[0] if w_layout == 0 else W.shape[1]
    y = torch.empty(rows, out_f, dtype=torch.float32, device=x.device)
    a = torch.empty(rows, dtype=torch.float32, device=x.device) if att is not None else None
    call("hscn_linear_fwd", ptr(x), ptr(W), ptr(bias), ptr(x2), ptr(W2), ptr(att), ptr(a), ptr(y),
         rows, in_f, out_f, w_layout, act, stream())
    return y, a


def linear_bwd_w_raw(gy: Tensor, x: Optional[Tensor], want_w: bool = True,
                     want_b: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    rows, out_f = gy.shape
    in_f = x.shape[1] if x is not None else 0
    dev = gy.device
    gW = torch.empty(out_f, in_f, dtype=torch.float32, device=dev) if (want_w and x is not None) else None
    gb = torch.empty(out_f, dtype=torch.float32, device=dev) if want_b else None
    nbytes = int(_hip.lib().hscn_linear_bwd_w_workspace_bytes(rows, in_f, out_f))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    call("hscn_linear_bwd_w", ptr(gy), ptr(x), ptr(gW), ptr(gb), rows, in_f, out_f, 0, ptr(ws), nbytes,
         stream())
    return gW, gb


def act_bwd_raw(gy: Tensor, y: Tensor, act: int) -> Tensor:
    if act == 0:
        return gy
    g = torch.empty_like(gy)
    call("hscn_act_bwd", ptr(gy), ptr(y), ptr(g), gy.numel(), act, stream())
    return g


def spmm_gcn_raw(csr: CSR, dinv_r: Tensor, dinv_c: Tensor, h: Tensor, bias: Optional[Tensor] = None,
                 act: int = 0) -> Tensor:
    out = torch.empty(csr.num_rows, h.shape[1], dtype=torch.float32, device=h.device)
    call("hscn_spmm_csr_gcn", ptr(csr.rowptr), ptr(csr.col), ptr(dinv_r), ptr(dinv_c), ptr(h), ptr(bias),
         ptr(out), csr.num_rows, h.shape[1], 0, act, stream())
    return out


def spmm_weighted_raw(csr: CSR, w: Optional[Tensor], x: Tensor) -> Tensor:
    out = torch.empty(csr.num_rows, x.shape[1], dtype=torch.float32, device=x.device)
    call("hscn_spmm_csr_weighted", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid) if w is not None else None,
         ptr(w), ptr(x), ptr(out), csr.num_rows, x.shape[1], stream())
    return out


# --------------------------------------------------------------------------- #
# Activation
# --------------------------------------------------------------------------- #
class ActFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, act: int):
        x = _c(x)
        y = torch.empty_like(x)
        call("hscn_act_fwd", ptr(x), ptr(y), x.numel(), act, stream())
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        (y,) = ctx.saved_tensors
        return act_bwd_raw(_c(g), y, ctx.act), None


class Activation:
    """Callable activation computed on the HIP path; ``hscn_name`` lets modules
    fuse it into the producing kernel's epilogue."""

    def __init__(self, name: str):
        self.hscn_name = name

    def __call__(self, x: Tensor) -> Tensor:
        if self.hscn_name == "identity":
            return x
        return ActFn.apply(x, ACT[self.hscn_name])

    def __repr__(self) -> str:
        return f"Activation({self.hscn_name})"


# --------------------------------------------------------------------------- #
# Dropout (MPNN baseline, reference model/mpnn.py:58)
# --------------------------------------------------------------------------- #
class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, p: float, seed: int):
        x = _c(x)
        y = torch.empty_like(x)
        call("hscn_dropout", ptr(x), ptr(y), x.numel(), float(p), int(seed), stream())
        ctx.p, ctx.seed = float(p), int(seed)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        g = _c(g)
        gx = torch.empty_like(g)
        call("hscn_dropout", ptr(g), ptr(gx), g.numel(), ctx.p, ctx.seed, stream())   # same seed: same mask
        return gx, None, None


_dropout_calls = 0


def dropout(x: Tensor, p: float = 0.5, training: bool = True, seed: Optional[int] = None) -> Tensor:
    """``F.dropout`` semantics (inverted scaling; identity when not training or p == 0).  The mask comes
    from the library's counter-based generator, keyed by ``seed`` (default: ``torch.initial_seed()`` mixed
    with a per-call counter, so ``torch.manual_seed`` makes a run repeatable); it is NOT the mask torch's
    own generator would draw.  The default seed is a host value: a captured hipGraph replays one mask."""
    if p < 0.0 or p > 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    if not training or p == 0.0:
        return x
    if p == 1.0:
        return x * 0.0
    if seed is None:
        seed = default_seed()
    return DropoutFn.apply(x, p, seed)


def default_seed() -> int:
    """The next seed of the host generator behind ``dropout``'s default: ``torch.initial_seed()`` mixed with a per-call
    counter (``nn.functional.LapPEDeepSetFn``'s sign flips draw from it too)."""
    global _dropout_calls
    _dropout_calls += 1
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _dropout_calls) & 0xFFFFFFFFFFFFFFFF


# --------------------------------------------------------------------------- #
# Linear
# --------------------------------------------------------------------------- #
class LinearFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, W: Tensor, bias: Optional[Tensor], act: int):
        x, W, bias = _c(x), _c(W), _c(bias)
        y, _ = linear_raw(x, W, bias, act=act)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, W, y)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        x, W, y = ctx.saved_tensors
        g = act_bwd_raw(_c(g), y, ctx.act)
        gx = linear_raw(g, W, w_layout=1)[0] if ctx.needs_input_grad[0] else None
        gW, gb = linear_bwd_w_raw(g, x, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return gx, gW, gb, None


def linear(x: Tensor, W: Tensor, bias: Optional[Tensor] = None, act: str = "identity") -> Tensor:
    lead = x.shape[:-1]
    y = LinearFn.apply(x.reshape(-1, x.shape[-1]), W, bias, ACT[act])
    return y.view(*lead, W.shape[0])


# --------------------------------------------------------------------------- #
# LapPE node encoder, DeepSet model (csrc/lappe.hip)
# --------------------------------------------------------------------------- #
LAPPE_MAX_FREQS = 64
LAPPE_MAX_LAYERS = 4
LAPPE_ENVELOPE = (f"1 <= max_freqs <= {LAPPE_MAX_FREQS}, dim_pe a multiple of 4 in [4, 32] and "
                  f"1 <= layers <= {LAPPE_MAX_LAYERS}")


def lappe_supported(max_freqs: int, dim_pe: int, layers: int) -> bool:
    """The kernels' envelope (include/hscn.h: hscn_lappe_supported), restated so that a config validates without the
    library; tests/test_lappe_host.py pins the two to each other."""
    return 1 <= max_freqs <= LAPPE_MAX_FREQS and 4 <= dim_pe <= 32 and dim_pe % 4 == 0 and 1 <= layers <= LAPPE_MAX_LAYERS


def lappe_widths(dim_pe: int, layers: int):
    """[2, 2 dim_pe, ..., 2 dim_pe, dim_pe]: the DeepSet chain's widths (``layers`` Linears)."""
    return [2] + [2 * dim_pe] * (layers - 1) + [dim_pe]


class LapPEDeepSetFn(Function):
    """``apply(vec, val, weights, biases, seed_or_None) -> pe_sum [N, dim_pe]``: the LapPE DeepSet chain and its masked
    sum over the frequencies as ONE launch (hscn_lappe_fwd); ``seed``: an int flips the sign of whole frequency columns
    by Philox (training), None leaves them.  Gradients go to ``weights`` / ``biases`` only, through hscn_lappe_bwd, which
    regenerates the signs from the seed; ``vec`` / ``val`` are constants and one that requires grad is refused."""

    @classmethod
    def apply(cls, vec: Tensor, val: Tensor, weights, biases, seed: Optional[int] = None) -> Tensor:
        weights, biases = list(weights), list(biases)
        for name, t in (("vec", vec), ("val", val)):
            if t.requires_grad:
                raise ValueError(f"LapPEDeepSetFn: {name} requires grad, but the Laplacian statistics are constants "
                                 "of this operator (gradients go to the parameters only)")
        if vec.dim() != 2 or vec.shape != val.shape:
            raise ValueError(f"LapPEDeepSetFn: vec and val must both be [N, max_freqs], got {tuple(vec.shape)} and "
                             f"{tuple(val.shape)}")
        if not weights or len(weights) != len(biases):
            raise ValueError("LapPEDeepSetFn: one bias per weight, at least one layer")
        L, dim_pe = len(weights), int(weights[-1].shape[0])
        if not lappe_supported(int(vec.shape[1]), dim_pe, L):
            raise ValueError(f"LapPEDeepSetFn: max_freqs={int(vec.shape[1])}, dim_pe={dim_pe}, layers={L} outside the "
                             f"kernel's envelope ({LAPPE_ENVELOPE})")
        widths = lappe_widths(dim_pe, L)
        for l, (W, b) in enumerate(zip(weights, biases)):
            if tuple(W.shape) != (widths[l + 1], widths[l]) or tuple(b.shape) != (widths[l + 1],):
                raise ValueError(f"LapPEDeepSetFn: layer {l} must be [{widths[l + 1]}, {widths[l]}] with a bias of "
                                 f"{widths[l + 1]}, got {tuple(W.shape)} and {tuple(b.shape)}")
        flat = [t for wb in zip(weights, biases) for t in wb]
        return super().apply(vec, val, None if seed is None else int(seed), *flat)

    @staticmethod
    def _table(params):
        import ctypes
        return (ctypes.c_void_p * len(params))(*[ptr(t) for t in params])

    @staticmethod
    def forward(ctx, vec: Tensor, val: Tensor, seed: Optional[int], *params: Tensor):
        vec, val = _c(vec), _c(val)
        params = [_c(t.detach()) for t in params]
        N, K = vec.shape
        L, dim_pe = len(params) // 2, int(params[-1].shape[0])
        out = torch.empty(N, dim_pe, dtype=torch.float32, device=vec.device)
        flip, seed = (0, 0) if seed is None else (1, seed & 0xFFFFFFFFFFFFFFFF)
        if N:
            call("hscn_lappe_fwd", ptr(vec), ptr(val), LapPEDeepSetFn._table(params), N, K, dim_pe, L, flip, seed,
                 ptr(out), stream())
        ctx.flip, ctx.seed = flip, seed
        ctx.save_for_backward(vec, val, *params)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        vec, val, *params = ctx.saved_tensors
        N, K = vec.shape
        L, dim_pe = len(params) // 2, int(params[-1].shape[0])
        total = sum(p.numel() for p in params)
        if N == 0:
            gflat = torch.zeros(total, dtype=torch.float32, device=vec.device)
        else:
            g = _c(g)
            gflat = torch.empty(total, dtype=torch.float32, device=vec.device)
            need = int(_hip.lib().hscn_lappe_workspace_floats(N, K, dim_pe, L))
            ws = torch.empty(max(need, 1), dtype=torch.float32, device=vec.device)
            call("hscn_lappe_bwd", ptr(vec), ptr(val), ptr(g), LapPEDeepSetFn._table(params), N, K, dim_pe, L, ctx.flip,
                 ctx.seed, ptr(gflat), ptr(ws), need, stream())
        grads, off = [], 0
        for i, p in enumerate(params):                 # g_params is flat in the parameters' own order and layout
            grads.append(gflat[off:off + p.numel()].view(p.shape) if ctx.needs_input_grad[3 + i] else None)
            off += p.numel()
        return (None, None, None, *grads)


# hscn_linear_fwd keeps the whole [O, I] weight in LDS and answers HSCN_E_UNSUPPORTED above 160 KB (csrc/linear.hip:
# `lds > 160 * 1024`); tests/test_attention_host.py pins the two values to each other through the library's answer
LINEAR_MAX_WEIGHT_BYTES = 160 * 1024


def linear_wide(x: Tensor, W: Tensor, bias: Optional[Tensor] = None, act: str = "identity") -> Tensor:
    """``linear`` for a weight beyond the kernel's LDS-resident image (in * out * 4 bytes > 160 KB, e.g. the packed
    [3D, D] attention projection from D = 117): the output columns are computed in chunks of whole weight rows, one
    ``linear`` each (the activation is element-wise, so it stays in the epilogue), and concatenated."""
    O, I = W.shape
    if I * O * 4 <= LINEAR_MAX_WEIGHT_BYTES:
        return linear(x, W, bias, act)
    step = (LINEAR_MAX_WEIGHT_BYTES // (4 * I)) // 4 * 4
    if step < 4:
        raise ValueError(f"linear: {I} input columns are beyond the kernel's envelope")
    parts = [linear(x, W[o:o + step], None if bias is None else bias[o:o + step], act) for o in range(0, O, step)]
    return torch.cat(parts, -1)


# --------------------------------------------------------------------------- #
# GCNConv (unit weights, add_self_loops=False)
# --------------------------------------------------------------------------- #
class GCNConvFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, W: Tensor, bias: Optional[Tensor], rel: Relation, act: int):
        x, W, bias = _c(x), _c(W), _c(bias)
        h, _ = linear_raw(x, W)
        out = spmm_gcn_raw(rel.csr, rel.dinv, rel.dinv, h, bias, act)
        ctx.rel, ctx.act, ctx.has_bias = rel, act, bias is not None
        ctx.save_for_backward(x, W, out)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, W, out = ctx.saved_tensors
        rel: Relation = ctx.rel
        g = act_bwd_raw(_c(g), out, ctx.act)
        gb = linear_bwd_w_raw(g, None, False, True)[1] if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        gx = gW = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gh = spmm_gcn_raw(rel.csr_t, rel.dinv, rel.dinv, g)
            if ctx.needs_input_grad[1]:
                gW = linear_bwd_w_raw(gh, x, True, False)[0]
            if ctx.needs_input_grad[0]:
                gx = linear_raw(gh, W, w_layout=1)[0]
        return gx, gW, gb, None, None


# --------------------------------------------------------------------------- #
# GCNII's layer, PyG GCN2Conv (csrc/gcn2.hip)
# --------------------------------------------------------------------------- #
GCN2_MIN_WIDTH = 4
GCN2_MAX_WIDTH = 512
GCN2_ENVELOPE = f"channels a multiple of 4 in [{GCN2_MIN_WIDTH}, {GCN2_MAX_WIDTH}]"
GCN2_ROW_TILE = 32                 # rows a workgroup of the forward owns at a time; with two weights (two LDS tiles):
GCN2_ROW_TILE_TWO = 16
GCN2_RESIDENT_BYTES = 96 * 1024    # tile(s) + whole weight(s) within this: the weight stays in LDS
GCN2_TWO_WG_BYTES = 80 * 1024      # a streamed panel is chosen to leave room for two workgroups a CU, where one does
GCN2_LDS_BYTES = 160 * 1024
GCN2_PANELS = (64, 32, 16)
GCN2_ACTS = ("identity", "relu")


def gcn2_supported(H: int) -> bool:
    """The kernel's envelope (include/hscn.h: hscn_gcn2_supported), restated so that a config validates without the
    library; tests/test_gcn2_host.py pins the two to each other."""
    return GCN2_MIN_WIDTH <= H <= GCN2_MAX_WIDTH and H % 4 == 0


def gcn2_plan(H: int, shared_weights: bool = True) -> dict:
    """What the forward launch chooses for width ``H`` (hscn_gcn2_plan's arithmetic; the host test pins the two):
    ``row_tile``, ``panel`` (weight columns in LDS at a time), ``resident`` (the whole weight stays in LDS) and ``lds``
    bytes."""
    if not gcn2_supported(H):
        raise ValueError(f"GCN2Conv: width H={H} outside the kernel's envelope ({GCN2_ENVELOPE})")
    nw = 1 if shared_weights else 2
    rt = GCN2_ROW_TILE if shared_weights else GCN2_ROW_TILE_TWO
    tiles = nw * rt * (H + 2) * 4
    hp32 = (H + 31) // 32 * 32
    if tiles + nw * H * hp32 * 4 <= GCN2_RESIDENT_BYTES:
        return {"row_tile": rt, "panel": hp32, "resident": True, "lds": tiles + nw * H * hp32 * 4}
    for budget in (GCN2_TWO_WG_BYTES, GCN2_LDS_BYTES):
        for pw in GCN2_PANELS:
            if tiles + nw * H * pw * 4 <= budget:
                return {"row_tile": rt, "panel": pw, "resident": False, "lds": tiles + nw * H * pw * 4}
    raise ValueError(f"GCN2Conv: no LDS plan for H={H}")


def gcn2_resident_max_width(shared_weights: bool = True) -> int:
    """The widest H whose weight(s) stay in LDS: the weight-panel edge (128; 96 with two weights)."""
    return max(H for H in range(GCN2_MIN_WIDTH, GCN2_MAX_WIDTH + 1, 4) if gcn2_plan(H, shared_weights)["resident"])


def _check_gcn2_coeffs(alpha, beta) -> Tuple[float, float]:
    for name, v in (("alpha", alpha), ("beta", beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"GCN2Conv: {name} must be a number, got {v!r}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"GCN2Conv: alpha must be in [0, 1], got {alpha!r}")
    if not 0.0 < float(beta) <= 1.0:
        raise ValueError(f"GCN2Conv: beta must be in (0, 1], got {beta!r}")
    return float(alpha), float(beta)


class GCN2ConvFn(Function):
    """``apply(x, x0, W1, W2_or_None, rel, alpha, beta, act) -> out [N, H]``: one GCNII layer over ``rel`` (the
    self-loop relation ``GCNConv`` builds, with its ``dinv``) as ONE launch (hscn_gcn2_fwd):

        p = A_hat x;   W2 None: h = (1 - alpha) p + alpha x0,  y = (1 - beta) h + beta h W1
                       else:    y = (1 - beta) ((1 - alpha) p + alpha x0) + beta ((1 - alpha) p W1 + alpha x0 W2)
        out = act(y)

    ``W1`` / ``W2`` are [H, H] in PyG's layout.  The backward is at most three calls: hscn_gcn2_bwd (the cotangent of y,
    the products with the transposed weights, the gradient of x0), hscn_gcn2_bwd_w (the weight gradients through
    ``linear``'s ordered two-stage reduction) and the gather over ``rel.csr_t`` (hscn_spmm_csr_gcn) for the gradient of
    x; only what ``needs_input_grad`` asks for is computed, and with ``alpha == 1`` the gradient of x is exact zeros
    without a gather."""

    @staticmethod
    def forward(ctx, x: Tensor, x0: Tensor, W1: Tensor, W2: Optional[Tensor], rel: Relation, alpha: float, beta: float,
                act: int):
        alpha, beta = _check_gcn2_coeffs(alpha, beta)
        if act not in (ACT["identity"], ACT["relu"]):
            raise ValueError(f"GCN2Conv: the epilogue is one of {GCN2_ACTS} (got code {act})")
        x, x0, W1, W2 = _c(x), _c(x0), _c(W1), _c(W2)
        if x.dim() != 2 or x0.shape != x.shape:
            raise ValueError(f"GCN2Conv: x and x0 must both be [N, H], got {tuple(x.shape)} and {tuple(x0.shape)}")
        N, H = x.shape
        if not gcn2_supported(H):
            raise ValueError(f"GCN2Conv: width H={H} outside the kernel's envelope ({GCN2_ENVELOPE})")
        for name, W in (("weight1", W1), ("weight2", W2)):
            if W is not None and tuple(W.shape) != (H, H):
                raise ValueError(f"GCN2Conv: {name} must be [{H}, {H}], got {tuple(W.shape)}")
        if N and (rel.num_src != N or rel.num_dst != N):
            raise ValueError(f"GCN2Conv: the relation is {rel.num_src} -> {rel.num_dst} nodes, x has {N} rows")
        out = torch.empty(N, H, dtype=torch.float32, device=x.device)
        h = torch.empty(N, H, dtype=torch.float32, device=x.device)
        if N:
            call("hscn_gcn2_fwd", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(rel.dinv), ptr(x), ptr(x0), ptr(W1), ptr(W2),
                 ptr(out), ptr(h), N, H, alpha, beta, act, stream())
        ctx.rel, ctx.alpha, ctx.beta, ctx.act, ctx.two = rel, alpha, beta, act, W2 is not None
        ctx.save_for_backward(x0, W1, W2, out, h)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x0, W1, W2, out, h = ctx.saved_tensors
        rel: Relation = ctx.rel
        N, H = out.shape
        need_x, need_x0, need_w1, need_w2 = ctx.needs_input_grad[:4]
        need_w2 = need_w2 and ctx.two
        dev = out.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        zeros = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        if N == 0:
            return (zeros(0, H) if need_x else None, zeros(0, H) if need_x0 else None, zeros(H, H) if need_w1 else None,
                    zeros(H, H) if need_w2 else None, None, None, None, None)
        g = _c(g)
        gather = need_x and ctx.alpha != 1.0
        gyb = new(N, H) if (need_w1 or need_w2) else None
        gp = new(N, H) if gather else None
        gx0 = new(N, H) if need_x0 else None
        if gyb is not None or gp is not None or gx0 is not None:
            call("hscn_gcn2_bwd", ptr(g), ptr(out), ptr(W1), ptr(W2), ptr(gyb), ptr(gp), ptr(gx0), N, H, ctx.alpha,
                 ctx.beta, ctx.act, stream())
        gW1 = gW2 = None
        if gyb is not None:
            gW1 = new(H, H) if need_w1 else None
            gW2 = new(H, H) if need_w2 else None
            nbytes = int(_hip.lib().hscn_gcn2_bwd_w_workspace_bytes(N, H))
            ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
            call("hscn_gcn2_bwd_w", ptr(gyb), ptr(h), ptr(x0) if need_w2 else None, ptr(gW1), ptr(gW2), N, H, ctx.alpha,
                 ptr(ws), nbytes, stream())
        gx = None
        if need_x:
            gx = spmm_gcn_raw(rel.csr_t, rel.dinv, rel.dinv, gp) if gather else zeros(N, H)
        return gx, gx0, gW1, gW2, None, None, None, None


# --------------------------------------------------------------------------- #
# GraphConv (edge-weighted sum aggregation)
# --------------------------------------------------------------------------- #
class GraphConvFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, edge_weight: Optional[Tensor], W_rel: Tensor, b_rel: Optional[Tensor],
                W_root: Tensor, rel: Relation, act: int):
        x, W_rel, b_rel, W_root = _c(x), _c(W_rel), _c(b_rel), _c(W_root)
        edge_weight = _c(edge_weight)
        agg = spmm_weighted_raw(rel.csr, edge_weight, x)
        y, _ = linear_raw(agg, W_rel, b_rel, x2=x, W2=W_root, act=act)
        ctx.rel, ctx.act, ctx.has_bias = rel, act, b_rel is not None
        ctx.save_for_backward(x, edge_weight, W_rel, W_root, agg, y)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        x, ew, W_rel, W_root, agg, y = ctx.saved_tensors
        rel: Relation = ctx.rel
        g = act_bwd_raw(_c(g), y, ctx.act)
        gW_rel, gb = linear_bwd_w_raw(g, agg, ctx.needs_input_grad[2], ctx.has_bias and ctx.needs_input_grad[3])
        gW_root = linear_bwd_w_raw(g, x, True, False)[0] if ctx.needs_input_grad[4] else None
        gx = None
        if ctx.needs_input_grad[0]:
            g_agg = linear_raw(g, W_rel, w_layout=1)[0]
            gx = spmm_weighted_raw(rel.csr_t, ew, g_agg)
            gx += linear_raw(g, W_root, w_layout=1)[0]
        # d/d edge_weight is not provided: gcn_norm weights are constants on this path
        return gx, None, gW_rel, gb, gW_root, None, None


# --------------------------------------------------------------------------- #
# GATConv, heads=1, bipartite, add_self_loops=False
# --------------------------------------------------------------------------- #
class GATConvFn(Function):
    @staticmethod
    def forward(ctx, x_src: Tensor, x_dst: Tensor, W_src: Tensor, W_dst: Tensor, att_src: Tensor,
                att_dst: Tensor, bias: Optional[Tensor], rel: Relation, slope: float, act: int):
        x_src, x_dst, W_src, W_dst, bias = _c(x_src), _c(x_dst), _c(W_src), _c(W_dst), _c(bias)
        att_s, att_d = _c(att_src).view(-1), _c(att_dst).view(-1)
        hs, a_s = linear_raw(x_src, W_src, att=att_s)
        hd, a_d = linear_raw(x_dst, W_dst, att=att_d)
        H = hs.shape[1]
        alpha = torch.empty(max(rel.num_edges, 1), dtype=torch.float32, device=hs.device)
        out = torch.empty(rel.num_dst, H, dtype=torch.float32, device=hs.device)
        call("hscn_gat_segment_fwd", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(a_s), ptr(a_d), ptr(hs),
             ptr(bias), ptr(alpha), ptr(out), rel.num_dst, H, float(slope), 0, act, stream())
        ctx.rel, ctx.act, ctx.slope, ctx.has_bias = rel, act, float(slope), bias is not None
        ctx.save_for_backward(x_src, x_dst, W_src, W_dst, att_s, att_d, hs, hd, a_s, a_d, alpha, out)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x_src, x_dst, W_src, W_dst, att_s, att_d, hs, hd, a_s, a_d, alpha, out = ctx.saved_tensors
        rel: Relation = ctx.rel
        H = hs.shape[1]
        dev = hs.device
        g = act_bwd_raw(_c(g), out, ctx.act)
        gb = linear_bwd_w_raw(g, None, False, True)[1] if (ctx.has_bias and ctx.needs_input_grad[6]) else None
        g_pre = torch.empty(max(rel.num_edges, 1), dtype=torch.float32, device=dev)
        g_a_d = torch.empty(rel.num_dst, dtype=torch.float32, device=dev)
        call("hscn_gat_segment_bwd_dst", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(a_s), ptr(a_d), ptr(hs),
             ptr(alpha), ptr(g), ptr(g_pre), ptr(g_a_d), rel.num_dst, H, ctx.slope, stream())
        g_a_s = torch.empty(rel.num_src, dtype=torch.float32, device=dev)
        g_hs = torch.empty(rel.num_src, H, dtype=torch.float32, device=dev)
        call("hscn_gat_segment_bwd_src", ptr(rel.csr_t.rowptr), ptr(rel.csr_t.col), ptr(rel.pos_t), ptr(alpha),
             ptr(g_pre), ptr(g), ptr(att_s), ptr(g_a_s), ptr(g_hs), rel.num_src, H, stream())
        g_att_s = linear_bwd_w_raw(g_a_s.view(-1, 1), hs, True, False)[0].view(1, 1, H)
        g_att_d = linear_bwd_w_raw(g_a_d.view(-1, 1), hd, True, False)[0].view(1, 1, H)
        gW_src = linear_bwd_w_raw(g_hs, x_src, True, False)[0] if ctx.needs_input_grad[2] else None
        gx_src = linear_raw(g_hs, W_src, w_layout=1)[0] if ctx.needs_input_grad[0] else None
        gW_dst = gx_dst = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            g_hd = linear_raw(g_a_d.view(-1, 1), att_d.view(H, 1))[0]
            if ctx.needs_input_grad[3]:
                gW_dst = linear_bwd_w_raw(g_hd, x_dst, True, False)[0]
            if ctx.needs_input_grad[1]:
                gx_dst = linear_raw(g_hd, W_dst, w_layout=1)[0]
        return gx_src, gx_dst, gW_src, gW_dst, g_att_s, g_att_d, gb, None, None, None


# --------------------------------------------------------------------------- #
# GATConv, heads=1, homogeneous, add_self_loops=True, one shared transform (the MPNN baseline's "gat")
# --------------------------------------------------------------------------- #
# Dispatch of GATLoopFn, per call: a relation whose largest raw in-degree is at most this takes the narrow-row
# kernels (csrc/gat_loops.hip, a lane group walks its row serially); above it the wave-per-row kernels of
# csrc/gat.hip run over the explicit-loop relation.  Either side is correct at any degree; the value is the
# measured crossover of forward + both backward launches on a Peptides-shaped batch of 128 with one hub row
# (profiles/r05_gat_mpnn.json: at 10 the narrow trio is ahead by more than the spread, at 18 behind).
GAT_NARROW_MAX_DEGREE = 10


class GATLoopFn(Function):
    """(x [N,F], W [H,F], att_src, att_dst, bias) -> act(GATConv(x, edge_index)) with PyG's self-loop handling.
    ``rel`` is the relation of the RAW edge list (input loops are skipped in the kernels, each node's own term is added
    last); ``rel_loops`` is None for the narrow-row kernels, or the relation over ``with_self_loops(edge_index)``
    for the wave-per-row kernels."""

    @staticmethod
    def forward(ctx, x: Tensor, W: Tensor, att_src: Tensor, att_dst: Tensor, bias: Optional[Tensor],
                rel: Relation, rel_loops: Optional[Relation], slope: float, act: int):
        x, W, bias = _c(x), _c(W), _c(bias)
        att_s, att_d = _c(att_src).view(-1), _c(att_dst).view(-1)
        h, a_s = linear_raw(x, W, att=att_s)
        H = h.shape[1]
        a_d = linear_raw(h, att_d.view(1, H))[0].view(-1)
        N, dev = h.shape[0], h.device
        out = torch.empty(N, H, dtype=torch.float32, device=dev)
        if rel_loops is None:
            kept = torch.empty(max(N, 1), 2, dtype=torch.float32, device=dev)          # row max, exp-sum
            call("hscn_gat_loop_fwd", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(a_s), ptr(a_d), ptr(h), ptr(bias),
                 ptr(kept), ptr(out), N, H, float(slope), act, stream())
        else:
            kept = torch.empty(max(rel_loops.num_edges, 1), dtype=torch.float32, device=dev)   # alpha per slot
            call("hscn_gat_segment_fwd", ptr(rel_loops.csr.rowptr), ptr(rel_loops.csr.col), ptr(a_s), ptr(a_d),
                 ptr(h), ptr(bias), ptr(kept), ptr(out), N, H, float(slope), 0, act, stream())
        ctx.rel, ctx.rel_loops = rel, rel_loops
        ctx.act, ctx.slope, ctx.has_bias = act, float(slope), bias is not None
        ctx.save_for_backward(x, W, att_s, att_d, h, a_s, a_d, kept, out)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, W, att_s, att_d, h, a_s, a_d, kept, out = ctx.saved_tensors
        rel: Relation = ctx.rel
        N, H = h.shape
        dev = h.device
        g = act_bwd_raw(_c(g), out, ctx.act)
        gb = linear_bwd_w_raw(g, None, False, True)[1] if (ctx.has_bias and ctx.needs_input_grad[4]) else None
        g_a = torch.empty(max(N, 1), 2, dtype=torch.float32, device=dev)    # {dL/da_src, dL/da_dst} per node
        g_h = torch.empty(N, H, dtype=torch.float32, device=dev)
        if ctx.rel_loops is None:
            tsum = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
            call("hscn_gat_loop_bwd_dst", ptr(rel.csr.rowptr), ptr(rel.csr.col), ptr(a_s), ptr(a_d), ptr(h),
                 ptr(kept), ptr(g), ptr(tsum), ptr(g_a), N, H, ctx.slope, stream())
            call("hscn_gat_loop_bwd_src", ptr(rel.csr_t.rowptr), ptr(rel.csr_t.col), ptr(a_s), ptr(a_d), ptr(h),
                 ptr(kept), ptr(tsum), ptr(g), ptr(att_s), ptr(att_d), ptr(g_a), ptr(g_h), N, H, ctx.slope, stream())
            g_att = linear_bwd_w_raw(g_a[:N], h, True, False)[0]            # [2, H]: both attention vectors at once
            g_att_s, g_att_d = g_att[0].view(1, 1, H), g_att[1].view(1, 1, H)
        else:
            lo: Relation = ctx.rel_loops
            g_pre = torch.empty(max(lo.num_edges, 1), dtype=torch.float32, device=dev)
            g_a_d = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
            g_a_s = torch.empty(max(N, 1), dtype=torch.float32, device=dev)
            call("hscn_gat_segment_bwd_dst", ptr(lo.csr.rowptr), ptr(lo.csr.col), ptr(a_s), ptr(a_d), ptr(h),
                 ptr(kept), ptr(g), ptr(g_pre), ptr(g_a_d), N, H, ctx.slope, stream())
            call("hscn_gat_segment_bwd_src", ptr(lo.csr_t.rowptr), ptr(lo.csr_t.col), ptr(lo.pos_t), ptr(kept),
                 ptr(g_pre), ptr(g), ptr(att_s), ptr(g_a_s), ptr(g_h), N, H, stream())
            g_h += linear_raw(g_a_d[:N].view(-1, 1), att_d.view(H, 1))[0]   # + g_a_dst (x) att_dst
            g_att_s = linear_bwd_w_raw(g_a_s[:N].view(-1, 1), h, True, False)[0].view(1, 1, H)
            g_att_d = linear_bwd_w_raw(g_a_d[:N].view(-1, 1), h, True, False)[0].view(1, 1, H)
        gW = linear_bwd_w_raw(g_h, x, True, False)[0] if ctx.needs_input_grad[1] else None
        gx = linear_raw(g_h, W, w_layout=1)[0] if ctx.needs_input_grad[0] else None
        return (gx, gW, g_att_s if ctx.needs_input_grad[2] else None, g_att_d if ctx.needs_input_grad[3] else None,
                gb, None, None, None, None)


# --------------------------------------------------------------------------- #
# GINEConv's aggregate: z_i = (1 + eps) x_i + sum_{k: dst_k = i} relu(x[src_k] + lin(edge_attr[k]))
# --------------------------------------------------------------------------- #
# csrc/gine.hip: a row of more than GINE_LONG_ROW slots (of either CSR: in-degree in the forward, out-degree in the
# backward's source walk) is summed by a whole workgroup in chunks of GINE_CHUNK slots; both are the library's
# constants (hscn_gine_long_row / hscn_gine_chunk, pinned equal in tests/test_edge_features_host.py).
GINE_LONG_ROW = 256
GINE_CHUNK = 64
GINE_MAX_WIDTH = 512
GINE_MAX_EDGE_DIM = 64


class GINEAggregateFn(Function):
    """(x [N, F], edge_attr [E, De], W [F, De], bias [F]) -> z [N, F] over ``rel`` (row k of ``edge_attr`` belongs to
    edge k of ``rel.edge_index``).  Forward: one launch; nothing but the inputs is kept.  Backward: the gates are
    recomputed; ``gx`` walks the source-keyed CSR and is computed only when ``x`` needs it; the gradients of ``W`` and
    ``bias`` go through gm [E, F] (plain stores) and the ordered ``hscn_linear_bwd_w``.  A gradient for ``edge_attr``
    does not exist and is refused, not returned as None."""

    @staticmethod
    def forward(ctx, x: Tensor, edge_attr: Tensor, W: Tensor, bias: Tensor, rel: Relation, eps: float):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError(
                "GINEConv: edge_attr requires a gradient (a trainable edge encoder in front of lin), which the "
                "operator does not compute: d edge_attr[k] = lin.weight^T (gate_k * gz[dst_k]) is not implemented")
        x, edge_attr, W, bias = _c(x), _c(edge_attr), _c(W), _c(bias)
        N, F = x.shape
        De = W.shape[1]
        if not _hip.lib().hscn_gine_supported(F, De):
            raise ValueError(f"GINEConv: width F={F}, edge_dim De={De} outside the kernel's envelope "
                             f"(1 <= F <= {GINE_MAX_WIDTH}, 1 <= De <= {GINE_MAX_EDGE_DIM})")
        if rel.num_src != N or rel.num_dst != N:
            raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, x has {N} rows")
        if edge_attr.dim() != 2 or edge_attr.size(0) != rel.num_edges or edge_attr.size(1) != De:
            raise ValueError(f"edge_attr is {tuple(edge_attr.shape)}; the relation has {rel.num_edges} edges and "
                             f"lin takes {De} edge features")
        if W.shape[0] != F or bias.shape != (F,):
            raise ValueError(f"lin maps to {W.shape[0]} columns, x has {F}")
        E = rel.num_edges
        csr = rel.csr
        z = torch.empty(N, F, dtype=torch.float32, device=x.device)
        call("hscn_gine_aggregate_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(x),
             ptr(edge_attr) if E else None, ptr(W), ptr(bias), float(eps), ptr(z), N, E, F, De, ptr(csr.flag), stream())
        ctx.rel, ctx.eps = rel, float(eps)
        ctx.save_for_backward(x, edge_attr, W, bias)
        return z

    @staticmethod
    def backward(ctx, gz: Tensor):
        x, edge_attr, W, bias = ctx.saved_tensors
        rel: Relation = ctx.rel
        gz = _c(gz)
        N, F = x.shape
        De, E = W.shape[1], rel.num_edges
        ea = ptr(edge_attr) if E else None
        gx = gW = gb = None
        if ctx.needs_input_grad[0]:
            t = rel.csr_t
            gx = torch.empty_like(x)
            call("hscn_gine_aggregate_bwd_x", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(x), ea, ptr(W), ptr(bias),
                 ctx.eps, ptr(gz), ptr(gx), N, E, F, De, ptr(rel.csr.flag), stream())
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            if E:
                gm = torch.empty(E, F, dtype=torch.float32, device=x.device)
                call("hscn_gine_aggregate_bwd_msg", ptr(rel.edge_index.contiguous()), ptr(x), ea, ptr(W), ptr(bias),
                     ptr(gz), ptr(gm), N, E, F, De, ptr(rel.csr.flag), stream())
                gW, gb = linear_bwd_w_raw(gm, edge_attr, ctx.needs_input_grad[2], ctx.needs_input_grad[3])
            else:                                   # no edge reaches lin: exact zeros, not None
                gW = torch.zeros_like(W) if ctx.needs_input_grad[2] else None
                gb = torch.zeros_like(bias) if ctx.needs_input_grad[3] else None
        return gx, None, gW, gb, None, None


# --------------------------------------------------------------------------- #
# PNAConv's aggregate: mean / min / max / sum / std of m_k = a[dst_k] + b[src_k] + t_k under degree scalers
# --------------------------------------------------------------------------- #
# csrc/pna.hip: the codes of include/hscn.h in the order of the library's enums; long rows as in GINE's aggregate
# (hscn_pna_long_row / hscn_pna_chunk, pinned equal in tests/test_pna_host.py).
PNA_AGGREGATORS = ("mean", "min", "max", "sum", "std")
PNA_SCALERS = ("identity", "amplification", "attenuation")
PNA_LONG_ROW = 256
PNA_CHUNK = 64
PNA_MAX_WIDTH = 512
PNA_ENVELOPE = (f"1 <= F <= {PNA_MAX_WIDTH}, aggregators a non-empty subset of {PNA_AGGREGATORS} and scalers a "
                f"non-empty subset of {PNA_SCALERS}")


def pna_supported(F: int, num_aggregators: int = 1, num_scalers: int = 1) -> bool:
    """hscn_pna_supported: the one statement of the kernel's envelope."""
    return bool(_hip.lib().hscn_pna_supported(int(F), int(num_aggregators), int(num_scalers)))


def pna_codes(aggregators, scalers):
    """The two name lists as the library's codes; a name outside the lists, a repeat or an empty list is a ValueError."""
    out = []
    for what, names, known in (("aggregators", aggregators, PNA_AGGREGATORS), ("scalers", scalers, PNA_SCALERS)):
        names = tuple(names)
        if not names:
            raise ValueError(f"PNA: {what} must name at least one of {known}")
        for n in names:
            if n not in known:
                raise ValueError(f"PNA: unknown entry {n!r} in {what}; known: {known}")
        if len(set(names)) != len(names):
            raise ValueError(f"PNA: {what} {names} repeats an entry")
        out.append(tuple(known.index(n) for n in names))
    return out[0], out[1]


def _codes_host(codes):
    import ctypes
    return (ctypes.c_int32 * len(codes))(*codes)


class PNAAggregateFn(Function):
    """(a [N, F], b [N, F], t [E, F] or None) -> [N, S A F] over ``rel`` (row k of ``t`` belongs to edge k of
    ``rel.edge_index``): the aggregators of the messages ``m_k = a[dst_k] + b[src_k] + t_k`` over every node's
    in-edges, each under every scaler, columns scaler-major, then aggregator-major, then F (PyG's
    ``DegreeScalerAggregation``).  ``aggregators`` / ``scalers``: names out of ``PNA_AGGREGATORS`` / ``PNA_SCALERS``;
    ``avg_deg_log``: the training set's mean of ``log(deg + 1)``, read by "amplification" and "attenuation" only.
    min / max ties go to the first slot of the row in CSR order, and the whole gradient with them.

    Forward: one launch; the [E, F] messages are never written.  Kept for backward: b, t and -- only what the named
    aggregators need -- the row means and stds [N, F] and the argmin / argmax edge ids [N, 2F].  Backward: one
    elementwise launch folds the scalers into the cotangent and gives ``g_a``; ``g_b`` walks the source-keyed CSR,
    ``g_t`` is edge-parallel; only what ``needs_input_grad`` asks for is computed.  No float atomics."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, t: Optional[Tensor], rel: Relation, aggregators, scalers,
                avg_deg_log: Optional[float] = None):
        aggr, scal = pna_codes(aggregators, scalers)
        for name, x in (("a", a), ("b", b), ("t", t)):
            if x is None:
                continue
            if x.dtype != torch.float32:
                raise TypeError(f"PNAAggregateFn: {name} must be float32, got {x.dtype}")
            if x.dim() != 2:
                raise ValueError(f"PNAAggregateFn: {name} must be 2-D, got {tuple(x.shape)}")
            if not x.is_contiguous():
                raise ValueError(f"PNAAggregateFn: {name} must be contiguous")
        N, F = a.shape
        if b.shape != a.shape:
            raise ValueError(f"PNAAggregateFn: b is {tuple(b.shape)}, a is {tuple(a.shape)}")
        if rel.num_src != N or rel.num_dst != N:
            raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, a has {N} rows")
        E = rel.num_edges
        if t is not None and tuple(t.shape) != (E, F):
            raise ValueError(f"PNAAggregateFn: t is {tuple(t.shape)}; the relation has {E} edges and the messages are "
                             f"{F} wide")
        if any(s != 0 for s in scal):
            if avg_deg_log is None or not (float(avg_deg_log) > 0.0 and float(avg_deg_log) < float("inf")):
                raise ValueError(f"PNAAggregateFn: scalers {tuple(scalers)} need a positive, finite avg_deg_log, got "
                                 f"{avg_deg_log!r}")
        if not pna_supported(F, len(aggr), len(scal)):
            raise ValueError(f"PNAAggregateFn: width F={F} outside the kernel's envelope ({PNA_ENVELOPE})")
        for name, x in (("a", a), ("b", b), ("t", t)):
            if x is not None and not x.is_cuda:
                raise RuntimeError(f"PNAAggregateFn takes HIP device tensors only ({name} is a CPU tensor): the hot "
                                   "path has no CPU fallback")
        need_a, need_b, need_t = ctx.needs_input_grad[:3]
        if (need_b or need_t) and rel._csr_t is None:
            raise ValueError("PNAAggregateFn: b or t requires a gradient and the relation carries the target-keyed CSR "
                             "only; build it with both=True (Relation(edge_index, N, N, both=True))")
        dev = a.device
        avg = float(avg_deg_log) if avg_deg_log is not None else 0.0
        keep = need_a or need_b or need_t
        walk = need_b or need_t
        out = torch.empty(N, len(scal) * len(aggr) * F, dtype=torch.float32, device=dev)
        has_std, has_arg = 4 in aggr, (1 in aggr or 2 in aggr)
        mean = torch.empty(N, F, dtype=torch.float32, device=dev) if (walk and has_std) else None
        std = torch.empty(N, F, dtype=torch.float32, device=dev) if (keep and has_std) else None
        arg = torch.empty(N, 2 * F, dtype=torch.int32, device=dev) if (walk and has_arg) else None
        csr = rel.csr
        call("hscn_pna_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(a), ptr(b), ptr(t), ptr(out), ptr(mean),
             ptr(std), ptr(arg), N, E, F, _codes_host(aggr), len(aggr), _codes_host(scal), len(scal), avg,
             ptr(csr.flag), stream())
        ctx.rel, ctx.spec = rel, (aggr, scal, avg)
        ctx.has_t = t is not None
        ctx.save_for_backward(b, t, mean, std, arg)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):
        b, t, mean, std, arg = ctx.saved_tensors
        rel: Relation = ctx.rel
        aggr, scal, avg = ctx.spec
        need_a, need_b, need_t = ctx.needs_input_grad[:3]
        g_out = _c(g_out)
        N, F = b.shape
        E = rel.num_edges
        dev = b.device
        gw = torch.empty(N, 4, F, dtype=torch.float32, device=dev)
        g_a = torch.empty(N, F, dtype=torch.float32, device=dev) if need_a else None
        call("hscn_pna_bwd_fold", ptr(rel.csr.rowptr), ptr(g_out), ptr(std), ptr(gw), ptr(g_a), N, F, _codes_host(aggr),
             len(aggr), _codes_host(scal), len(scal), avg, stream())
        g_b = g_t = None
        if need_b:
            ct = rel.csr_t
            g_b = torch.empty(N, F, dtype=torch.float32, device=dev)
            call("hscn_pna_bwd_src", ptr(ct.rowptr), ptr(ct.col), ptr(ct.eid), ptr(b), ptr(t), ptr(gw), ptr(mean),
                 ptr(arg), ptr(g_b), N, E, F, ptr(rel.csr.flag), stream())
        if need_t and ctx.has_t:
            g_t = torch.empty(E, F, dtype=torch.float32, device=dev)
            call("hscn_pna_bwd_edge", ptr(rel.edge_index.contiguous()) if E else None, ptr(b), ptr(t), ptr(gw),
                 ptr(mean), ptr(arg), ptr(g_t), N, E, F, ptr(rel.csr.flag), stream())
        return g_a, g_b, g_t, None, None, None, None


# --------------------------------------------------------------------------- #
# GatedGCN's aggregate: e^_k = Dx_i + Ex_j + Ce_k, h_i = Ax_i + sum_k s_k Bx_j / (sum_k s_k + 1e-6), s = sigmoid(e^)
# --------------------------------------------------------------------------- #
# csrc/gatedgcn.hip: a row of more than GATEDGCN_LONG_ROW slots (in-degree in the forward and the backward's target
# walk, out-degree in the source walk) is summed by a whole workgroup in chunks of GATEDGCN_CHUNK slots; both are the
# library's constants (hscn_gatedgcn_long_row / hscn_gatedgcn_chunk, pinned equal in tests/test_gatedgcn_host.py).
GATEDGCN_LONG_ROW = 256
GATEDGCN_CHUNK = 64
GATEDGCN_MAX_WIDTH = 512


def gatedgcn_supported(H: int) -> bool:
    return bool(_hip.lib().hscn_gatedgcn_supported(int(H)))


def _source_grads(E: int, a: Tensor, b: Tensor, need_a: bool, need_b: bool, walk):
    """The two gradients of a source-keyed walk, each like its operand, None where not needed: ``walk(ga, gb)`` fills
    them when the relation has edges; otherwise no edge reaches the operands: exact zeros, not None."""
    new = torch.empty_like if E else torch.zeros_like
    ga, gb = new(a) if need_a else None, new(b) if need_b else None
    if E and (need_a or need_b):
        walk(ga, gb)
    return ga, gb


class GatedGCNAggregateFn(Function):
    """(Ax, Bx, Dx, Ex [N, H], Ce [E, H]) -> (h [N, H], e_out [E, H]) over ``rel``, with j = src_k, i = dst_k; row k
    of ``Ce`` and ``e_out`` belongs to edge k of ``rel.edge_index``.  Forward: one launch; kept for backward are Ax, Bx,
    the two outputs and den [N, H] (the per-node sum of gates).  Backward: the gates are recomputed from ``e_out``; the
    target-keyed pass gives the gradients of Ce and Dx, the source-keyed pass (``rel.csr_t``, built only then) those of
    Bx and Ex; the gradient of Ax is the cotangent of h.  Only what ``needs_input_grad`` asks for is computed; a
    cotangent that autograd leaves out (the edge output of a stack's last layer) is not materialised."""

    @staticmethod
    def forward(ctx, Ax: Tensor, Bx: Tensor, Dx: Tensor, Ex: Tensor, Ce: Tensor, rel: Relation):
        Ax, Bx, Dx, Ex, Ce = _c(Ax), _c(Bx), _c(Dx), _c(Ex), _c(Ce)
        if Ax.dim() != 2:
            raise ValueError(f"GatedGCNConv: Ax must be [N, H], got {tuple(Ax.shape)}")
        N, H = Ax.shape
        if not _hip.lib().hscn_gatedgcn_supported(H):
            raise ValueError(f"GatedGCNConv: width H={H} outside the kernel's envelope (1 <= H <= {GATEDGCN_MAX_WIDTH})")
        for name, t in (("Bx", Bx), ("Dx", Dx), ("Ex", Ex)):
            if t.shape != Ax.shape:
                raise ValueError(f"GatedGCNConv: {name} is {tuple(t.shape)}, Ax is {tuple(Ax.shape)}")
        if rel.num_src != N or rel.num_dst != N:
            raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, x has {N} rows")
        E = rel.num_edges
        if Ce.dim() != 2 or Ce.size(0) != E or Ce.size(1) != H:
            raise ValueError(f"Ce is {tuple(Ce.shape)}; the relation has {E} edges and the layer is {H} wide")
        csr = rel.csr
        dev = Ax.device
        h = torch.empty(N, H, dtype=torch.float32, device=dev)
        den = torch.empty(N, H, dtype=torch.float32, device=dev)
        e_out = torch.empty(E, H, dtype=torch.float32, device=dev)
        call("hscn_gatedgcn_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid),
             ptr(rel.edge_index.contiguous()) if E else None, ptr(Ax), ptr(Bx), ptr(Dx), ptr(Ex),
             ptr(Ce) if E else None, ptr(h), ptr(e_out) if E else None, ptr(den), N, E, H, ptr(csr.flag), stream())
        ctx.rel = rel
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(Ax, Bx, h, e_out, den)
        return h, e_out

    @staticmethod
    def backward(ctx, gh: Optional[Tensor], ge_out: Optional[Tensor]):
        Ax, Bx, h, e_out, den = ctx.saved_tensors
        rel: Relation = ctx.rel
        N, H = Ax.shape
        E = rel.num_edges
        need_a, need_b, need_d, need_e, need_c = ctx.needs_input_grad[:5]
        gh = torch.zeros_like(Ax) if gh is None else _c(gh)
        ge_out = _c(ge_out)
        gBx = gDx = gEx = ge = None
        edges = need_d or need_e or need_c
        if edges or need_b:
            csr = rel.csr
            gn = torch.empty_like(Ax)
            if edges:
                ge = torch.empty(E, H, dtype=torch.float32, device=Ax.device)
                gDx = torch.empty_like(Ax)
            call("hscn_gatedgcn_bwd_dst", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid),
                 ptr(rel.edge_index.contiguous()) if E else None, ptr(Ax), ptr(Bx), ptr(h), ptr(e_out) if E else None,
                 ptr(den), ptr(gh), ptr(ge_out) if (E and ge_out is not None) else None, ptr(gn),
                 ptr(ge) if (E and edges) else None, ptr(gDx), N, E, H, ptr(csr.flag), stream())

            def walk(gBx, gEx):
                t = rel.csr_t
                call("hscn_gatedgcn_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(e_out), ptr(gn), ptr(ge),
                     ptr(gBx), ptr(gEx), N, E, H, ptr(csr.flag), stream())

            gBx, gEx = _source_grads(E, Ax, Ax, need_b, need_e, walk)
        return (gh if need_a else None, gBx, gDx if need_d else None, gEx, ge if need_c else None, None)


# --------------------------------------------------------------------------- #
# Edge attention (TransformerConv's message + aggregate): multi-head softmax(q_i . (k_j + e_k) / sqrt(C)) over in-edges
# --------------------------------------------------------------------------- #
# csrc/edge_attention.hip: a row of more than EDGE_ATTN_LONG_ROW slots (in-degree in the forward and the backward's
# target walk, out-degree in the source walk) is taken by a whole workgroup in chunks of EDGE_ATTN_CHUNK slots; both
# are the library's constants (hscn_edge_attn_long_row / hscn_edge_attn_chunk, pinned equal in
# tests/test_transformerconv_host.py).
EDGE_ATTN_LONG_ROW = 256
EDGE_ATTN_CHUNK = 64
EDGE_ATTN_MAX_WIDTH = 512
EDGE_ATTN_ENVELOPE = f"heads >= 1, head width >= 1 and heads * head width <= {EDGE_ATTN_MAX_WIDTH}"


def edge_attn_supported(heads: int, head_dim: int) -> bool:
    """hscn_edge_attn_supported: the one statement of the kernel's envelope."""
    return bool(_hip.lib().hscn_edge_attn_supported(int(heads), int(head_dim)))


def _head_attention_dims(op: str, operands, heads: int, shapes, supported, envelope: str):
    """What both sparse attention operators check of their named ``operands`` (the first is q) -> (rows, HC, C): float32
    and 2-D, ``heads | width``, then ``shapes(rows, HC)`` -- the operator's own checks of its relation or structure --
    then the kernel's envelope and the device.  ``op`` names the operator in every message."""
    for name, t in operands:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{op}: {name} must be float32, got {t.dtype}")
        if t is not None and t.dim() != 2:
            raise ValueError(f"{op}: {name} must be 2-D [rows, heads * C], got {tuple(t.shape)}")
    rows, HC = operands[0][1].shape
    if heads < 1 or HC % heads:
        raise ValueError(f"{op}: width {HC} is not a multiple of heads = {heads}")
    C = HC // heads
    shapes(rows, HC)
    if not supported(heads, C):
        raise ValueError(f"{op}: heads = {heads}, head width = {C} outside the kernel's envelope ({envelope})")
    for _, t in operands:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{op} takes HIP device tensors only (got a CPU tensor): the hot path has no CPU fallback")
    return rows, HC, C


class EdgeAttentionFn(Function):
    """(q [Nd, Hd*C], k, v [Ns, Hd*C], e [E, Hd*C] or None) -> out [Nd, Hd*C] over ``rel`` (j = src_k, i = dst_k; row k
    of ``e`` belongs to edge k of ``rel.edge_index``): per head, ``out_i = sum_k softmax_k(q_i . (k_j + e_k) / sqrt(C))
    (v_j + e_k)`` over the in-edges of i, zeros for a node without any.  Forward: one launch; kept for backward are
    the inputs, the output and ONE log-sum-exp per (node, head), as its two summands (row maximum, log of the shifted
    sum) -- the attention weights are recomputed, never stored.
    Backward: the target-keyed pass gives dq, de and the per-(node, head) ``sum(dout * out)``; the source-keyed pass
    (``rel.csr_t``, built only then) gives dk and dv.  Only what ``needs_input_grad`` asks for is computed."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, e: Optional[Tensor], rel: Relation, heads: int):
        heads = int(heads)
        E = rel.num_edges

        def shapes(Nd, HC):
            if k.shape != v.shape or k.size(1) != HC:
                raise ValueError(f"edge attention: k is {tuple(k.shape)}, v is {tuple(v.shape)}, q is {tuple(q.shape)}")
            if rel.num_src != k.size(0) or rel.num_dst != Nd:
                raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, k has {k.size(0)} rows and q "
                                 f"has {Nd}")
            if e is not None and (e.size(0) != E or e.size(1) != HC):
                raise ValueError(f"e is {tuple(e.shape)}; the relation has {E} edges and the layer is {HC} wide")

        Nd, HC, C = _head_attention_dims("edge attention", (("q", q), ("k", k), ("v", v), ("e", e)), heads, shapes,
                                         edge_attn_supported, EDGE_ATTN_ENVELOPE)
        Ns = k.size(0)
        q, k, v, e = _c(q), _c(k), _c(v), _c(e)
        csr = rel.csr
        dev = q.device
        out = torch.empty(Nd, HC, dtype=torch.float32, device=dev)
        lse = torch.empty(Nd, heads, 2, dtype=torch.float32, device=dev)   # (row maximum, log of the shifted sum)
        call("hscn_edge_attn_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(q), ptr(k), ptr(v),
             ptr(e) if E else None, ptr(out), ptr(lse), Nd, Ns, E, heads, C, ptr(csr.flag), stream())
        ctx.rel, ctx.heads = rel, heads
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, e, out, lse)
        return out

    @staticmethod
    def backward(ctx, go: Optional[Tensor]):
        q, k, v, e, out, lse = ctx.saved_tensors
        rel: Relation = ctx.rel
        heads = ctx.heads
        need_q, need_k, need_v, need_e = ctx.needs_input_grad[:4]
        need_e = need_e and e is not None
        if go is None or not (need_q or need_k or need_v or need_e):
            return None, None, None, None, None, None
        go = _c(go)
        Nd, HC = q.shape
        Ns, E, C = k.size(0), rel.num_edges, HC // heads
        csr = rel.csr
        delta = torch.empty(Nd, heads, dtype=torch.float32, device=q.device)
        dq = torch.empty_like(q) if need_q else None
        de = torch.empty_like(e) if need_e else None
        call("hscn_edge_attn_bwd_dst", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(q), ptr(k), ptr(v),
             ptr(e) if E else None, ptr(out), ptr(lse), ptr(go), ptr(delta), ptr(dq), ptr(de) if E else None,
             Nd, Ns, E, heads, C, ptr(csr.flag), stream())

        def walk(dk, dv):
            t = rel.csr_t
            call("hscn_edge_attn_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(q), ptr(k), ptr(v), ptr(e),
                 ptr(lse), ptr(delta), ptr(go), ptr(dk), ptr(dv), Nd, Ns, E, heads, C, ptr(csr.flag), stream())

        dk, dv = _source_grads(E, k, v, need_k, need_v, walk)
        return dq, dk, dv, de, None, None


# --------------------------------------------------------------------------- #
# Exphormer: expander edges (csrc/expander.hip) and typed sparse attention over the union graph (csrc/exphormer.hip)
# --------------------------------------------------------------------------- #
EXPANDER_MAX_NODES = 2048
EXPANDER_MAX_DEGREE = 32
EXPANDER_GRAPH_TOO_LARGE = 1      # flag bit 0: a graph with more than max_nodes nodes (its edges are -1)
EXPH_MAX_VIRTUAL_NODES = 4
EXPH_MAX_WIDTH = 512
EXPH_ENVELOPE = f"heads >= 1, head width >= 1 and heads * head width <= {EXPH_MAX_WIDTH}"

_EXPANDER_FLAGS = _hip.FlagWord()


def expander_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every expander launch ORs into; ``check_expander`` reads and clears it."""
    return _EXPANDER_FLAGS.of(device)


def check_expander(device) -> None:
    """Synchronising: ``ValueError`` if an expander launch since the last check met a graph larger than the
    ``max_nodes`` it was given (that graph's edges are -1, the other graphs' are as always)."""
    f = _EXPANDER_FLAGS.take(device)
    if f & EXPANDER_GRAPH_TOO_LARGE:
        raise ValueError("expander_edges: a graph has more nodes than max_nodes says (or than the kernel's "
                         f"{EXPANDER_MAX_NODES}); its expander edges are -1")


def expander_edges(ptr32: Tensor, degree: int, seed: int, graph_ids: Optional[Tensor] = None, *, max_nodes: int,
                   num_nodes: Optional[int] = None) -> Tensor:
    """Exphormer's expander for every graph of a batch (``hscn_expander_build``, one launch): int64 [2, degree * N],
    graph g's ``n_g * degree`` edges at column ``degree * ptr32[g]`` -- ``degree / 2`` random Hamiltonian cycles in both
    directions, drawn from Philox under ``seed`` and the graph's id (``graph_ids[g]``, or g): a graph's expander does
    not depend on its place in the batch.  Loops (n = 1) and repeats (n = 2) are kept.  ``num_nodes``: N on the host
    (``Batch.num_nodes``); without it ``ptr32[-1]`` is read back once.  No CPU fallback."""
    degree, max_nodes = int(degree), int(max_nodes)
    if degree < 2 or degree % 2 or degree > EXPANDER_MAX_DEGREE:
        raise ValueError(f"expander_edges: degree must be even in [2, {EXPANDER_MAX_DEGREE}], got {degree}")
    if not 0 <= max_nodes <= EXPANDER_MAX_NODES:
        raise ValueError(f"expander_edges: a graph of {max_nodes} nodes is outside the kernel's envelope (one graph's "
                         f"sort keys in LDS: at most {EXPANDER_MAX_NODES} nodes)")
    if ptr32.dtype != torch.int32 or ptr32.dim() != 1 or ptr32.numel() < 1:
        raise TypeError("ptr32 must be an int32 [B + 1] tensor (graph_hscn.data.Batch.ptr32)")
    if not ptr32.is_cuda:
        raise RuntimeError("expander_edges takes HIP device tensors only (got a CPU tensor): there is no CPU "
                           "fallback -- move the batch to the device")
    B = ptr32.numel() - 1
    dev = ptr32.device
    if graph_ids is not None:
        if graph_ids.dim() != 1 or graph_ids.numel() != B or graph_ids.is_floating_point():
            raise ValueError(f"graph_ids must be {B} integers, one per graph")
        if graph_ids.device != dev:
            raise RuntimeError(f"graph_ids is on {graph_ids.device}, ptr32 on {dev}")
        graph_ids = graph_ids.to(torch.int32).contiguous()
    N = int(ptr32[-1].item()) if num_nodes is None else int(num_nodes)
    out = torch.empty(2, degree * N, dtype=torch.int64, device=dev)
    call("hscn_expander_build", ptr(ptr32.contiguous()), ptr(graph_ids), N, B, degree, int(seed) & (2 ** 64 - 1),
         max_nodes, ptr(out) if N else None, ptr(expander_flags(dev)), stream())
    return out


def exph_attn_supported(heads: int, head_dim: int) -> bool:
    """hscn_exph_attn_supported: the one statement of the kernel's envelope."""
    return bool(_hip.lib().hscn_exph_attn_supported(int(heads), int(head_dim)))


class ExphormerAttentionFn(Function):
    """(q, k, v [N', Hd*C], e_edge [E_local, Hd*C] or None, e_type [T, Hd*C]) -> out [N', Hd*C] over the union graph of
    ``struct`` (``structure.ExphormerStructure``): per head ``w_k = exp(clamp(q_i . (k_j * e_k) / sqrt(C), -5, 5))`` and
    ``out_i = sum_k w_k v_j / (sum_k w_k + 1e-6)`` over the in-edges of i, zeros for a row without any.  ``e_k`` is row
    ``erow[k]`` of ``e_edge`` or row ``erow[k] - E_local`` of ``e_type``.  Forward: one launch; kept are the inputs, the
    output and ONE float per (row, head), the sum of the weights -- the weights are recomputed, never stored.
    Backward: the target-keyed pass gives dq, de_edge and the per-(row, head) ``sum(dout * out)``; the source-keyed pass
    gives dk and dv; the type-keyed pass gives de_type, every type's slots summed in fixed chunks in list order (two
    launches, no float atomics).  Only what ``needs_input_grad`` asks for is computed."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, e_edge: Optional[Tensor], e_type: Tensor, struct, heads: int):
        heads = int(heads)
        El, T, E = struct.num_edge_rows, struct.num_types, struct.num_edges

        def shapes(N, HC):
            if k.shape != q.shape or v.shape != q.shape:
                raise ValueError(f"exphormer attention: k is {tuple(k.shape)}, v is {tuple(v.shape)}, q is "
                                 f"{tuple(q.shape)}")
            if struct.num_rows != N:
                raise ValueError(f"the union graph has {struct.num_rows} rows (nodes + virtual nodes), q has {N}")
            if e_edge is None and El:
                raise ValueError(f"the union graph names {El} per-edge feature rows and e_edge is None")
            if e_edge is not None and (e_edge.size(0) != El or e_edge.size(1) != HC):
                raise ValueError(f"e_edge is {tuple(e_edge.shape)}; the union graph names {El} per-edge rows and the "
                                 f"layer is {HC} wide")
            if e_type.size(0) != T or e_type.size(1) != HC:
                raise ValueError(f"e_type is {tuple(e_type.shape)}; the union graph has {T} edge types and the layer is "
                                 f"{HC} wide")

        operands = (("q", q), ("k", k), ("v", v), ("e_edge", e_edge), ("e_type", e_type))
        N, HC, C = _head_attention_dims("exphormer attention", operands, heads, shapes, exph_attn_supported, EXPH_ENVELOPE)
        q, k, v, e_edge, e_type = _c(q), _c(k), _c(v), _c(e_edge), _c(e_type)
        csr = struct.rel.csr
        dev = q.device
        out = torch.empty(N, HC, dtype=torch.float32, device=dev)
        z = torch.empty(N, heads, dtype=torch.float32, device=dev)
        call("hscn_exph_attn_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(struct.erow), ptr(q), ptr(k),
             ptr(v), ptr(e_edge) if El else None, ptr(e_type), ptr(out), ptr(z), N, E, El, T, heads, C, ptr(csr.flag),
             stream())
        ctx.struct, ctx.heads = struct, heads
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, k, v, e_edge, e_type, out, z)
        return out

    @staticmethod
    def backward(ctx, go: Optional[Tensor]):
        q, k, v, e_edge, e_type, out, z = ctx.saved_tensors
        struct, heads = ctx.struct, ctx.heads
        need_q, need_k, need_v, need_e, need_t = ctx.needs_input_grad[:5]
        need_e = need_e and e_edge is not None
        if go is None or not (need_q or need_k or need_v or need_e or need_t):
            return None, None, None, None, None, None, None
        go = _c(go)
        N, HC = q.shape
        C = HC // heads
        El, T, E = struct.num_edge_rows, struct.num_types, struct.num_edges
        rel = struct.rel
        csr = rel.csr
        delta = torch.empty(N, heads, dtype=torch.float32, device=q.device)
        dq = torch.empty_like(q) if need_q else None
        # every e_edge row is named by exactly one union edge (the structure checks it): each row is written once
        de = torch.empty_like(e_edge) if need_e else None
        dt = None
        call("hscn_exph_attn_bwd_dst", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(struct.erow), ptr(q), ptr(k),
             ptr(v), ptr(e_edge) if El else None, ptr(e_type), ptr(out), ptr(z), ptr(go), ptr(delta), ptr(dq),
             ptr(de) if El else None, N, E, El, T, heads, C, ptr(csr.flag), stream())

        def walk(dk, dv):
            t = rel.csr_t
            call("hscn_exph_attn_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(struct.erow), ptr(q), ptr(k),
                 ptr(v), ptr(e_edge) if El else None, ptr(e_type), ptr(z), ptr(delta), ptr(go), ptr(dk), ptr(dv),
                 N, E, El, T, heads, C, ptr(csr.flag), stream())

        dk, dv = _source_grads(E, k, v, need_k, need_v, walk)
        if need_t:
            dt = torch.empty_like(e_type)
            trowptr, titem = struct.type_slots
            ws_bytes = int(_hip.lib().hscn_exph_type_workspace_bytes(E, T, heads, C))
            ws = torch.empty(max(ws_bytes // 4, 4), dtype=torch.float32, device=q.device)
            call("hscn_exph_attn_bwd_type", ptr(trowptr), ptr(titem), ptr(struct.edge_index) if E else None, ptr(q),
                 ptr(k), ptr(v), ptr(e_type), ptr(z), ptr(delta), ptr(go), ptr(dt), N, E, T, heads, C, ptr(csr.flag),
                 ptr(ws), ws.numel() * 4, stream())
        return dq, dk, dv, de, dt, None, None


# --------------------------------------------------------------------------- #
# SAN: full-graph attention over real and fake edges (csrc/san.hip)
# --------------------------------------------------------------------------- #
SAN_MIN_HEAD_DIM = 4
SAN_MAX_HEAD_DIM = 64
SAN_MAX_WIDTH = 512
SAN_MAX_NODES = 4096
SAN_EDGE_OUT_OF_GRAPH = 1         # flag bit 0: an edge with an end outside its target's graph (skipped; the pair is fake)
SAN_GRAPH_TOO_LARGE = 2           # flag bit 1: a graph with more than max_nodes nodes (its rows are NaN)
SAN_ENVELOPE = (f"head width a multiple of 4 in [{SAN_MIN_HEAD_DIM}, {SAN_MAX_HEAD_DIM}], heads >= 1, heads * head "
                f"width <= {SAN_MAX_WIDTH}, graphs of at most {SAN_MAX_NODES} nodes")

_SAN_FLAGS = _hip.FlagWord()


def san_attn_supported(heads: int, head_dim: int, max_nodes: int = 0) -> bool:
    """hscn_san_attn_supported: the one statement of the kernel's envelope."""
    return bool(_hip.lib().hscn_san_attn_supported(int(heads), int(head_dim), int(max_nodes)))


def san_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every SAN attention launch ORs into; ``check_san`` reads and clears it."""
    return _SAN_FLAGS.of(device)


def check_san(device) -> None:
    """Synchronising: ``ValueError`` if a SAN attention launch since the last check met an edge that names a node
    outside its target's graph (the edge was skipped and the pair counted as fake) or a graph larger than the
    ``max_nodes`` it was given (that graph's rows are NaN)."""
    f = _SAN_FLAGS.take(device)
    if f & SAN_EDGE_OUT_OF_GRAPH:
        raise ValueError("SAN attention: an edge names a node outside its target's graph (or an edge id outside the "
                         "edge list); it was skipped and the pair counted as fake")
    if f & SAN_GRAPH_TOO_LARGE:
        raise ValueError("SAN attention: a graph has more nodes than the batch's max_nodes says; its rows are NaN")


def _check_gamma(gamma) -> float:
    gamma = float(gamma)
    if not (gamma >= 0.0 and gamma != float("inf")):
        raise ValueError(f"SAN attention: gamma must be finite and >= 0, got {gamma!r}")
    return gamma


class SANAttentionFn(Function):
    """(q, k, v [N, Hd*C], e [E, Hd*C], q2, k2e [N, Hd*C] or None) -> (out [N, Hd*C], z [N, Hd]) over ``rel`` (j =
    src_x, i = dst_x; row x of ``e`` belongs to edge x of ``rel.edge_index``) and the graphs of ``ptr32``: per head every
    listed edge j -> i inside a graph weighs ``a exp(clamp(q_i . (k_j * e_x) / sqrt(C), -5, 5))``, every other ordered
    pair (j, i) of a graph, j = i included, ``b exp(clamp(q2_i . k2e_j / sqrt(C), -5, 5))`` with ``a = 1 / (1 + gamma)``,
    ``b = gamma / (1 + gamma)``; ``z`` is the sum of a row's weights and ``out = sum w v_j / (z + 1e-6)``.
    ``full_graph=False``: the edges alone with a = 1 (``q2`` and ``k2e`` are None), zeros for a node without in-edges.
    Forward: one launch; kept are the inputs, ``out`` and ``z`` -- the weights are recomputed, never stored.  Backward:
    the query-keyed pass gives dq, de, dq2 and the per-(row, head) ``sum(dout * out)``, the key-keyed pass (``rel.csr_t``,
    built only then) dk, dv and dk2e.  Only what ``needs_input_grad`` asks for is computed; ``z`` carries no gradient."""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, e: Tensor, q2: Optional[Tensor], k2e: Optional[Tensor],
                rel: Relation, ptr32: Tensor, max_nodes: int, heads: int, gamma: float, full_graph: bool):
        heads, max_nodes, full_graph = int(heads), int(max_nodes), bool(full_graph)
        gamma = _check_gamma(gamma) if full_graph else 0.0
        E = rel.num_edges
        if e is None:
            raise ValueError("SAN attention: e is None; every edge needs a feature row (e must be [E, heads * C])")
        if full_graph and (q2 is None or k2e is None):
            raise ValueError("SAN attention: full_graph needs q2 and k2e")
        if not full_graph and (q2 is not None or k2e is not None):
            raise ValueError("SAN attention: q2 and k2e belong to full_graph=True (pass None)")

        def shapes(N, HC):
            for name, t in (("k", k), ("v", v), ("q2", q2), ("k2e", k2e)):
                if t is not None and t.shape != q.shape:
                    raise ValueError(f"SAN attention: {name} is {tuple(t.shape)}, q is {tuple(q.shape)}")
            if rel.num_src != N or rel.num_dst != N:
                raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, q has {N} rows")
            if e.size(0) != E or e.size(1) != HC:
                raise ValueError(f"e is {tuple(e.shape)}; the relation has {E} edges (one row per edge) and the layer "
                                 f"is {HC} wide")
            if ptr32.dtype != torch.int32 or ptr32.dim() != 1 or ptr32.numel() < 1:
                raise TypeError("ptr32 must be an int32 [B + 1] tensor (graph_hscn.data.Batch.ptr32)")
            if max_nodes < 0:
                raise ValueError(f"max_nodes must be >= 0, got {max_nodes}")

        operands = (("q", q), ("k", k), ("v", v), ("e", e), ("q2", q2), ("k2e", k2e))
        N, HC, C = _head_attention_dims("SAN attention", operands, heads, shapes,
                                        lambda h, c: san_attn_supported(h, c, max_nodes), SAN_ENVELOPE)
        if ptr32.device != q.device:
            raise RuntimeError(f"ptr32 is on {ptr32.device}, q on {q.device}: move the batch to the device once")
        q, k, v, e, q2, k2e = _c(q), _c(k), _c(v), _c(e), _c(q2), _c(k2e)
        ptr32 = ptr32.contiguous()
        B = ptr32.numel() - 1
        csr = rel.csr
        dev = q.device
        out = torch.empty(N, HC, dtype=torch.float32, device=dev)
        z = torch.empty(N, heads, dtype=torch.float32, device=dev)
        call("hscn_san_attn_fwd", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(ptr32), ptr(q), ptr(k), ptr(v),
             ptr(e) if E else None, ptr(q2), ptr(k2e), ptr(out), ptr(z), N, E, B, max_nodes, heads, C, gamma,
             int(full_graph), ptr(san_flags(dev)), stream())
        ctx.rel, ctx.dims = rel, (N, E, B, max_nodes, heads, C, gamma, full_graph)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(z)
        ctx.save_for_backward(q, k, v, e, q2, k2e, ptr32, out, z)
        return out, z

    @staticmethod
    def backward(ctx, go: Optional[Tensor], _gz=None):
        q, k, v, e, q2, k2e, ptr32, out, z = ctx.saved_tensors
        rel: Relation = ctx.rel
        N, E, B, max_nodes, heads, C, gamma, full = ctx.dims
        need_q, need_k, need_v, need_e, need_q2, need_k2 = ctx.needs_input_grad[:6]
        need_q2, need_k2 = need_q2 and full, need_k2 and full
        none = (None,) * 12
        if go is None or not (need_q or need_k or need_v or need_e or need_q2 or need_k2):
            return none
        go = _c(go)
        csr = rel.csr
        flag = san_flags(q.device)
        delta = torch.empty(N, heads, dtype=torch.float32, device=q.device)
        # without edges no real pair reaches q: exact zeros; de: a skipped edge's row is not written
        dq = (torch.empty_like(q) if E else torch.zeros_like(q)) if need_q else None
        de = torch.zeros_like(e) if need_e else None
        dq2 = torch.empty_like(q2) if need_q2 else None
        tail = (N, E, B, max_nodes, heads, C, gamma, int(full), ptr(flag), stream())
        call("hscn_san_attn_bwd_dst", ptr(csr.rowptr), ptr(csr.col), ptr(csr.eid), ptr(ptr32), ptr(q), ptr(k), ptr(v),
             ptr(e) if E else None, ptr(q2), ptr(k2e), ptr(out), ptr(z), ptr(go), ptr(delta), ptr(dq),
             ptr(de) if E else None, ptr(dq2), *tail)
        dk = dv = dk2 = None
        if need_k or need_v or need_k2:
            # dk is the real term's alone (zeros without edges); dv and dk2e also see the fake pairs
            dk = (torch.empty_like(k) if E else torch.zeros_like(k)) if need_k else None
            dv = (torch.empty_like(v) if (E or full) else torch.zeros_like(v)) if need_v else None
            dk2 = torch.empty_like(k2e) if need_k2 else None
            if E or full:
                t = rel.csr_t
                call("hscn_san_attn_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(ptr32), ptr(q), ptr(k),
                     ptr(v), ptr(e) if E else None, ptr(q2), ptr(k2e), ptr(z), ptr(delta), ptr(go), ptr(dk), ptr(dv),
                     ptr(dk2), *tail)
        return (dq, dk, dv, de, dq2, dk2) + (None,) * 6


# --------------------------------------------------------------------------- #
# Global attention: block-diagonal multi-head self-attention over a batch (csrc/attention.hip)
# --------------------------------------------------------------------------- #
ATTN_MIN_HEAD_DIM = 4
ATTN_MAX_HEAD_DIM = 64
ATTN_MAX_WIDTH = 512
ATTN_GRAPH_TOO_LARGE = 4          # flag bit 2: a graph with more than max_nodes nodes (its rows are NaN)
ATTN_ENVELOPE = (f"head width embed_dim / num_heads a multiple of 4 in [{ATTN_MIN_HEAD_DIM}, {ATTN_MAX_HEAD_DIM}], "
                 f"num_heads >= 1, embed_dim <= {ATTN_MAX_WIDTH}")

_ATTN_FLAGS = _hip.FlagWord()


def attention_supported(heads: int, head_dim: int) -> bool:
    return bool(_hip.lib().hscn_attention_supported(int(heads), int(head_dim)))


def attention_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every attention launch ORs into; ``check_attention`` reads and clears it."""
    return _ATTN_FLAGS.of(device)


def check_attention(device) -> None:
    """Synchronising: ``ValueError`` if an attention launch since the last check met a graph larger than the
    ``max_nodes`` it was given (that graph's rows are NaN)."""
    f = _ATTN_FLAGS.take(device)
    if f & ATTN_GRAPH_TOO_LARGE:
        raise ValueError("self-attention: a graph has more nodes than the batch's max_nodes says; its rows are NaN")
    if f & 8:           # ATTN_BUCKETS_OUT_OF_RANGE (the biased operator below)
        raise ValueError("biased self-attention: a graph's bucket range lies outside the bucket tensor (the SPDBuckets "
                         "belong to another batch); its rows are NaN")


def _attention_dims(qkv: Tensor, ptr32: Tensor, heads: int, operands):
    """What both attention operators check of ``qkv`` and ``ptr32`` -> (N, D, dh, B).  ``operands(dh)`` holds the
    operator's own checks (the envelope, its further arguments); it runs between those of ``qkv`` and of ``ptr32``,
    raises, or answers the (name, tensor) pairs that must sit on ``qkv``'s device beside ``ptr32``."""
    if qkv.dim() != 2 or qkv.size(1) % (3 * heads) != 0:
        raise ValueError(f"qkv must be [N, 3 * heads * head_dim], got {tuple(qkv.shape)} for {heads} heads")
    N, D = qkv.size(0), qkv.size(1) // 3
    dh = D // heads
    others = operands(dh)
    if ptr32.dtype != torch.int32 or ptr32.dim() != 1 or ptr32.numel() < 1:
        raise TypeError("ptr32 must be an int32 [B + 1] tensor (graph_hscn.data.Batch.ptr32)")
    for name, t in (("ptr32", ptr32), *others):
        if t.device != qkv.device:
            raise RuntimeError(f"{name} is on {t.device}, qkv on {qkv.device}: move the batch to the device once "
                               "(Batch.to); the operator does not copy it on every call")
    return N, D, dh, ptr32.numel() - 1


class SelfAttentionFn(Function):
    """(qkv [N, 3D], ptr32 [B + 1] int32, max_nodes, heads) -> out [N, D]: every node attends to the nodes of its own
    graph.  Forward: one launch; ``qkv``, ``out`` and the rows' log-sum-exp are kept.  Backward: two launches (the Q
    third of ``g_qkv`` keyed by query, the K and V thirds keyed by key), only when ``qkv`` needs a gradient."""

    @staticmethod
    def forward(ctx, qkv: Tensor, ptr32: Tensor, max_nodes: int, heads: int):
        qkv = _c(qkv)

        def operands(dh):
            if not attention_supported(heads, dh):
                raise ValueError(f"self-attention: {heads} heads of width {dh} are outside the kernel's envelope "
                                 f"({ATTN_ENVELOPE})")
            return ()

        N, D, dh, B = _attention_dims(qkv, ptr32, heads, operands)
        out = torch.empty(N, D, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(N, heads, dtype=torch.float32, device=qkv.device)
        flag = attention_flags(qkv.device) if qkv.is_cuda else None
        call("hscn_attention_fwd", ptr(qkv), ptr(ptr32), N, B, int(max_nodes), heads, dh, ptr(out), ptr(lse),
             ptr(flag), stream())
        ctx.dims = (N, B, int(max_nodes), heads, dh)
        ctx.save_for_backward(qkv, ptr32, out, lse)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        qkv, ptr32, out, lse = ctx.saved_tensors
        N, B, max_nodes, heads, dh = ctx.dims
        g_out = _c(g_out)
        g_qkv = torch.empty_like(qkv)
        delta = torch.empty_like(lse)
        flag = attention_flags(qkv.device)
        call("hscn_attention_bwd_q", ptr(qkv), ptr(out), ptr(lse), ptr(g_out), ptr(ptr32), N, B, max_nodes, heads, dh,
             ptr(g_qkv), ptr(delta), ptr(flag), stream())
        call("hscn_attention_bwd_kv", ptr(qkv), ptr(lse), ptr(delta), ptr(g_out), ptr(ptr32), N, B, max_nodes, heads,
             dh, ptr(g_qkv), ptr(flag), stream())
        return g_qkv, None, None, None


# --------------------------------------------------------------------------- #
# Shortest-path buckets (csrc/spd.hip) and the self-attention they bias (csrc/attention.hip, BiasArgs): Graphormer's
# spatial encoding inside the global attention
# --------------------------------------------------------------------------- #
SPD_MIN_DIST = 1
SPD_MAX_DIST = 63
SPD_EDGE_OUT_OF_RANGE = 1         # flag bit 0: an edge with an end outside its graph (skipped)
SPD_GRAPH_TOO_LARGE = 2           # flag bit 1: a graph with more than max_nodes nodes (its buckets are all max_dist)
ATTN_MAX_BUCKETS = 64
ATTN_BUCKETS_OUT_OF_RANGE = 8     # attention flag bit 3: a graph's bucket range leaves the bucket tensor (rows NaN)

_SPD_FLAGS = _hip.FlagWord()


def spd_supported(max_nodes: int, max_dist: int) -> bool:
    """hscn_spd_supported: the one statement of the bucket kernel's envelope (a host function: no device needed)."""
    return bool(_hip.lib().hscn_spd_supported(int(max_nodes), int(max_dist)))


def spd_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every bucket launch ORs into; ``check_spd`` reads and clears it."""
    return _SPD_FLAGS.of(device)


def check_spd(device) -> None:
    """Synchronising: ``ValueError`` if a bucket launch since the last check met an edge with an end outside its graph
    (skipped) or a graph larger than the ``max_nodes`` it was given (all its buckets are ``max_dist``)."""
    f = _SPD_FLAGS.take(device)
    if f & SPD_EDGE_OUT_OF_RANGE:
        raise ValueError("shortest_path_buckets: an edge has an end outside its graph's node range; it was skipped")
    if f & SPD_GRAPH_TOO_LARGE:
        raise ValueError("shortest_path_buckets: a graph has more nodes than max_nodes says; its buckets are all max_dist")


class SPDBuckets:
    """What ``shortest_path_buckets`` answers: ``bucket`` [sum n_g^2] uint8 (graph g's [n_g, n_g] matrix row-major, row =
    query, column = key, at ``spd_ptr[g]``), ``spd_ptr`` [B + 1] int64 on the same device, and the ``max_dist`` and
    ``max_nodes`` it was built with.  ``max_dist + 1`` bucket values."""
    __slots__ = ("bucket", "spd_ptr", "max_dist", "max_nodes")

    def __init__(self, bucket: Tensor, spd_ptr: Tensor, max_dist: int, max_nodes: int):
        self.bucket, self.spd_ptr, self.max_dist, self.max_nodes = bucket, spd_ptr, int(max_dist), int(max_nodes)

    @property
    def num_buckets(self) -> int:
        return self.max_dist + 1

    def __repr__(self) -> str:
        return (f"SPDBuckets(bucket=[{self.bucket.numel()}], graphs={self.spd_ptr.numel() - 1}, "
                f"max_dist={self.max_dist}, max_nodes={self.max_nodes})")


def shortest_path_buckets(batch, max_dist: int, *, sizes=None) -> SPDBuckets:
    """Shortest-path distance buckets of every graph of a collated batch (``hscn_spd_buckets``): ``bucket(i, j)`` = the
    fewest edges on a directed path i -> j where that is below ``max_dist``, ``max_dist`` otherwise.

    ``batch``: a ``graph_hscn.data.Batch`` on the device, or the tuple ``(edge_index, ptr32, eptr32, max_nodes)``.  The
    layout needs every graph's node count ON THE HOST: ``train.batching.to_device`` takes them from the collated
    batch's ``ptr`` while it is on the host and keeps them beside the device copy; with a tuple, or a batch moved
    otherwise, pass ``sizes`` (a sequence of ints).  Nothing is read back from the device.  No CPU fallback."""
    max_dist = int(max_dist)
    if not SPD_MIN_DIST <= max_dist <= SPD_MAX_DIST:
        raise ValueError(f"shortest_path_buckets: max_dist must be in [{SPD_MIN_DIST}, {SPD_MAX_DIST}], got {max_dist}")
    if isinstance(batch, (tuple, list)):
        if len(batch) != 4:
            raise ValueError("shortest_path_buckets takes a Batch or (edge_index, ptr32, eptr32, max_nodes)")
        edge_index, ptr32, eptr32, max_nodes = batch
    else:
        for attr in ("edge_index", "ptr32", "eptr32", "max_nodes"):
            if not hasattr(batch, attr):
                raise ValueError(f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)")
        edge_index, ptr32, eptr32, max_nodes = batch.edge_index, batch.ptr32, batch.eptr32, batch.max_nodes
        if sizes is None:
            sizes = getattr(batch, "__dict__", {}).get("_host_sizes")
    max_nodes = int(max_nodes)
    if not spd_supported(max_nodes, max_dist):
        raise ValueError(f"shortest_path_buckets: a graph of {max_nodes} nodes is outside the kernel's envelope (adjacency "
                         "and two reachability bitsets of one graph within 160 KB of LDS: at most 646 nodes)")
    if sizes is None:
        raise ValueError("shortest_path_buckets needs every graph's node count on the host: a Batch moved by "
                         "train.batching.to_device carries them, otherwise pass sizes=[n_0, n_1, ...]")
    sizes = [int(n) for n in sizes]
    B = ptr32.numel() - 1
    if len(sizes) != B or any(n < 0 for n in sizes):
        raise ValueError(f"shortest_path_buckets: {len(sizes)} sizes for {B} graphs")
    if ptr32.dtype != torch.int32 or eptr32.dtype != torch.int32 or eptr32.numel() != B + 1:
        raise TypeError("ptr32 and eptr32 must be int32 [B + 1] tensors (graph_hscn.data.Batch)")
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise TypeError("edge_index must be an int64 [2, E] tensor")
    dev = ptr32.device
    if not ptr32.is_cuda:
        raise RuntimeError("shortest_path_buckets takes HIP device tensors only (got a CPU tensor): there is no CPU "
                           "fallback -- move the batch to the device")
    if edge_index.device != dev or eptr32.device != dev:
        raise RuntimeError(f"edge_index is on {edge_index.device}, eptr32 on {eptr32.device}, ptr32 on {dev}")
    host_ptr = torch.zeros(B + 1, dtype=torch.int64)
    if B:
        host_ptr[1:] = torch.cumsum(torch.as_tensor(sizes, dtype=torch.int64) ** 2, 0)
    total = int(host_ptr[-1])
    spd_ptr = host_ptr.to(dev)
    bucket = torch.empty(total, dtype=torch.uint8, device=dev)
    edge_index = edge_index.contiguous()
    N, E = sum(sizes), int(edge_index.size(1))
    call("hscn_spd_buckets", ptr(edge_index) if E else None, ptr(ptr32), ptr(eptr32), ptr(spd_ptr), N, E, B, total,
         max_nodes, max_dist, ptr(bucket) if total else None, ptr(spd_flags(dev)), stream())
    return SPDBuckets(bucket, spd_ptr, max_dist, max_nodes)


def attention_bias_supported(heads: int, head_dim: int, num_buckets: int) -> bool:
    return bool(_hip.lib().hscn_attention_bias_supported(int(heads), int(head_dim), int(num_buckets)))


class BiasedSelfAttentionFn(Function):
    """(qkv [N, 3D], table [num_buckets, heads], spd: SPDBuckets, ptr32, max_nodes, heads) -> out [N, D]:
    ``SelfAttentionFn`` with ``table[bucket_ij, h]`` added to the logit of query i and key j in head h.  Forward: one
    launch.  Backward: the query-keyed launch where ``qkv`` or ``table`` needs a gradient (with the table's ordered
    fold behind it where ``table`` does), the key-keyed launch where ``qkv`` does.  No host read anywhere."""

    @staticmethod
    def forward(ctx, qkv: Tensor, table: Tensor, spd: SPDBuckets, ptr32: Tensor, max_nodes: int, heads: int):
        qkv, table = _c(qkv), _c(table)

        def operands(dh):
            if not isinstance(spd, SPDBuckets):
                raise TypeError("spd must be the SPDBuckets nn.functional.shortest_path_buckets answers")
            if table.dim() != 2 or table.size(1) != heads or table.size(0) != spd.num_buckets:
                raise ValueError(f"biased self-attention: the table must be [{spd.num_buckets}, {heads}] (max_dist + 1 "
                                 f"buckets by heads), got {tuple(table.shape)}")
            if not attention_bias_supported(heads, dh, int(table.size(0))):
                raise ValueError(f"biased self-attention: {heads} heads of width {dh} with {table.size(0)} buckets are "
                                 f"outside the kernel's envelope ({ATTN_ENVELOPE}, at most {ATTN_MAX_BUCKETS} buckets)")
            return ("table", table), ("spd.bucket", spd.bucket), ("spd.spd_ptr", spd.spd_ptr)

        N, D, dh, B = _attention_dims(qkv, ptr32, heads, operands)
        nb = int(table.size(0))
        if spd.spd_ptr.numel() != B + 1:
            raise ValueError(f"spd holds {spd.spd_ptr.numel() - 1} graphs, ptr32 {B}")
        total = int(spd.bucket.numel())
        out = torch.empty(N, D, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(N, heads, dtype=torch.float32, device=qkv.device)
        flag = attention_flags(qkv.device) if qkv.is_cuda else None
        call("hscn_attention_bias_fwd", ptr(qkv), ptr(table), ptr(spd.bucket) if total else None, ptr(spd.spd_ptr),
             ptr(ptr32), N, B, total, int(max_nodes), heads, dh, nb, ptr(out), ptr(lse), ptr(flag), stream())
        ctx.dims = (N, B, total, int(max_nodes), heads, dh, nb)
        ctx.save_for_backward(qkv, table, spd.bucket, spd.spd_ptr, ptr32, out, lse)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):
        need_qkv, need_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_qkv or need_table):
            return None, None, None, None, None, None
        qkv, table, bucket, spd_ptr, ptr32, out, lse = ctx.saved_tensors
        N, B, total, max_nodes, heads, dh, nb = ctx.dims
        g_out = _c(g_out)
        g_qkv = torch.empty_like(qkv) if need_qkv else None
        delta = torch.empty_like(lse)
        g_table = work = None
        floats = 0
        if need_table:
            g_table = torch.empty_like(table)
            tile = int(_hip.lib().hscn_attention_tile())
            floats = B * max(1, -(-max_nodes // tile)) * heads * nb
            work = torch.empty(max(floats, 1), dtype=torch.float32, device=qkv.device)
        flag = attention_flags(qkv.device)
        pb = ptr(bucket) if total else None
        call("hscn_attention_bias_bwd_q", ptr(qkv), ptr(out), ptr(lse), ptr(g_out), ptr(table), pb, ptr(spd_ptr),
             ptr(ptr32), N, B, total, max_nodes, heads, dh, nb, ptr(g_qkv), ptr(delta), ptr(g_table), ptr(work), floats,
             ptr(flag), stream())
        if need_qkv:
            call("hscn_attention_bias_bwd_kv", ptr(qkv), ptr(lse), ptr(delta), ptr(g_out), ptr(table), pb, ptr(spd_ptr),
                 ptr(ptr32), N, B, total, max_nodes, heads, dh, nb, ptr(g_qkv), ptr(flag), stream())
        return g_qkv, g_table, None, None, None, None


# --------------------------------------------------------------------------- #
# Categorical encoders: out[i] = sum_c W[off_c + idx[i, c]] in column order (csrc/catenc.hip)
# --------------------------------------------------------------------------- #
# the kernels' envelope (hscn_catenc_supported; pinned equal in tests/test_categorical_host.py)
CATENC_MAX_WIDTH = 512
CATENC_MAX_COLUMNS = 16
CATENC_MAX_ROWS = 4096
CATENC_ENVELOPE = (f"emb_dim a multiple of 4 in [4, {CATENC_MAX_WIDTH}], at most {CATENC_MAX_COLUMNS} columns, "
                   f"at most {CATENC_MAX_ROWS} categories in all")
CATENC_BAD_INDEX = 1              # flag bit 0: an index outside [0, cardinality) of its column (its term is skipped)

_CATENC_FLAGS = _hip.FlagWord()


def catenc_supported(D: int, F: int, R: int) -> bool:
    """``hscn_catenc_supported`` restated on the host (a module is built before any device is touched)."""
    return (4 <= D <= CATENC_MAX_WIDTH and D % 4 == 0 and 1 <= F <= CATENC_MAX_COLUMNS and F <= R <= CATENC_MAX_ROWS)


def categorical_flags(device) -> Tensor:
    """The device's flag word [1] int32 that every categorical-encoder launch ORs into; ``check_categorical`` reads
    and clears it."""
    return _CATENC_FLAGS.of(device)


def check_categorical(device) -> None:
    """Synchronising: ``IndexError`` if a categorical-encoder launch since the last check met an index outside
    [0, cardinality) of its column (the term was skipped, nothing was read out of bounds)."""
    if _CATENC_FLAGS.take(device):
        raise IndexError("categorical encoder: a feature holds an index outside [0, cardinality) of its column "
                         "(its embedding was left out of the sum)")


def categorical_embed_reference(weight: Tensor, idx: Tensor, cardinalities) -> Tensor:
    """The plain-torch restatement (OGB's loop): ``index_select`` per column out of the column's own block (so that
    torch's bounds check is the column's), added in column order."""
    out, off = 0, 0
    for c, card in enumerate(cardinalities):
        out = out + weight.narrow(0, off, int(card)).index_select(0, idx[:, c])
        off += int(card)
    return out


class CategoricalEmbedFn(Function):
    """(weight [R, D], idx int64 [n, F], cardinalities) -> out [n, D] = sum_c weight[off_c + idx[i, c]], the adds in
    column order.  On a CPU weight it is ``categorical_embed_reference`` with autograd's own backward (the oracle of
    the tests).  On the device: one gather launch; the backward builds the ``CategoryIndex`` of ``idx`` (cached per
    tensor) and sums each table row's cotangent rows in item order -- no float atomics, the same bits every run."""

    @staticmethod
    def forward(ctx, weight: Tensor, idx: Tensor, cardinalities):
        cards = tuple(int(c) for c in cardinalities)
        if idx.dtype != torch.int64:
            raise TypeError(f"categorical features must be int64, got {idx.dtype}")
        if weight.dim() != 2 or idx.dim() != 2 or idx.size(1) != len(cards) or weight.size(0) != sum(cards):
            raise ValueError(f"weight {tuple(weight.shape)} / idx {tuple(idx.shape)} do not fit the cardinalities "
                             f"{cards} (weight [{sum(cards)}, D], idx [n, {len(cards)}])")
        ctx.cards = cards
        if not weight.is_cuda:
            with torch.enable_grad():
                w = weight.detach().requires_grad_(True)
                out = categorical_embed_reference(w, idx, cards)
            ctx.cpu = (w, out)
            return out.detach()
        n, F, (R, D) = int(idx.size(0)), len(cards), weight.shape
        if not _hip.lib().hscn_catenc_supported(D, F, R):
            raise ValueError(f"categorical encoder: D={D}, F={F}, R={R} outside the kernel's envelope ({CATENC_ENVELOPE})")
        if idx.device != weight.device:
            raise RuntimeError(f"idx is on {idx.device}, the table on {weight.device}")
        weight = _c(weight)
        out = torch.empty(n, D, dtype=torch.float32, device=weight.device)
        call("hscn_catenc_fwd", ptr(weight), ptr(idx.contiguous()) if n else None, host_cards(cards), ptr(out), n, F, D,
             ptr(categorical_flags(weight.device)), stream())
        ctx.idx = idx
        ctx.dims = (n, F, R, D)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        if hasattr(ctx, "cpu"):
            w, out = ctx.cpu
            return torch.autograd.grad(out, w, g_out)[0], None, None
        n, F, R, D = ctx.dims
        index = category_index_of(ctx.idx, ctx.cards)
        g_out = _c(g_out)
        gW = torch.empty(R, D, dtype=torch.float32, device=g_out.device)
        ws_bytes = int(_hip.lib().hscn_catenc_bwd_workspace_bytes(n, F, R, D))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g_out.device)
        call("hscn_catenc_bwd", ptr(index.rowptr), ptr(index.item), ptr(g_out) if n else None, ptr(gW), n, F, R, D,
             ptr(categorical_flags(g_out.device)), ptr(ws), ws_bytes, stream())
        return gW, None, None


def categorical_embed(weight: Tensor, idx: Tensor, cardinalities) -> Tensor:
    return CategoricalEmbedFn.apply(weight, idx, tuple(cardinalities))


# --------------------------------------------------------------------------- #
# global_mean_pool
# --------------------------------------------------------------------------- #
class SegmentMeanFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, seg: CSR, batch: Tensor, identity_nodes: bool):
        x = _c(x)
        out = torch.empty(seg.num_rows, x.shape[1], dtype=torch.float32, device=x.device)
        call("hscn_segment_mean_fwd", ptr(seg.rowptr), None if identity_nodes else ptr(seg.col), ptr(x),
             ptr(out), seg.num_rows, x.shape[1], stream())
        ctx.seg = seg
        ctx.save_for_backward(batch)
        ctx.n = x.shape[0]
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (batch,) = ctx.saved_tensors
        g = _c(g)
        gx = torch.empty(ctx.n, g.shape[1], dtype=torch.float32, device=g.device)
        call("hscn_segment_mean_bwd", ptr(ctx.seg.rowptr), ptr(batch), ptr(g), ptr(gx), ctx.n, g.shape[1],
             stream())
        return gx, None, None, None


# --------------------------------------------------------------------------- #
# MinCUT pooling losses on the edge-list route
# --------------------------------------------------------------------------- #
class MinCutSparseFn(Function):
    """(logits, x) -> (S, losses[2] = {mincut, ortho}, pooled_x, pooled_adj).
    Gradients flow from the two losses to ``logits`` (the only gradients the
    reference's stage A uses: model/hscn.py:63 discards out/out_adj)."""

    @staticmethod
    def forward(ctx, logits: Tensor, x: Optional[Tensor], rel: Relation, node_ptr: Tensor, num_graphs: int):
        logits, x = _c(logits), _c(x)
        n, K = logits.shape
        dev = logits.device
        Fx = x.shape[1] if x is not None else 0
        S = torch.empty_like(logits)
        stats = torch.empty(num_graphs, 4, dtype=torch.float32, device=dev)
        ss = torch.empty(num_graphs, K, K, dtype=torch.float32, device=dev)
        px = torch.empty(num_graphs, K, max(Fx, 1), dtype=torch.float32, device=dev) if x is not None else None
        padj = torch.empty(num_graphs, K, K, dtype=torch.float32, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        row_csr = rel.csr_t  # keyed by edge ROW (= source side of edge_index)
        call("hscn_mincut_sparse_fwd", ptr(logits), ptr(x), ptr(row_csr.rowptr), ptr(row_csr.col),
             ptr(node_ptr), ptr(S), ptr(stats), ptr(ss), ptr(px), ptr(padj), ptr(losses), n, num_graphs, K, Fx,
             stream())
        ctx.rel, ctx.G = rel, num_graphs
        ctx.save_for_backward(S, stats, ss, node_ptr)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(S, padj)
        if px is not None:
            ctx.mark_non_differentiable(px)
        return S, losses[0], losses[1], px, padj

    @staticmethod
    def backward(ctx, gS, g_mc, g_o, g_px, g_padj):
        S, stats, ss, node_ptr = ctx.saved_tensors
        rel: Relation = ctx.rel
        dev = S.device
        gl = _pack_loss_grads(g_mc, g_o, dev)
        g_logits = torch.empty_like(S)
        row_csr, col_csr = rel.csr_t, rel.csr
        call("hscn_mincut_sparse_bwd", ptr(S), ptr(stats), ptr(ss), ptr(row_csr.rowptr), ptr(row_csr.col),
             ptr(col_csr.rowptr), ptr(col_csr.col), ptr(node_ptr), ptr(gl), ptr(g_logits), S.shape[0], ctx.G,
             S.shape[1], stream())
        return g_logits, None, None, None, None


def _pack_loss_grads(g_mc: Optional[Tensor], g_o: Optional[Tensor], dev, *more: Optional[Tensor]) -> Tensor:
    """[dL/dmincut, dL/dortho] as one device pair: the two losses are separate autograd outputs (slicing
    one [2] output costs six fill / copy / add launches in the backward), packing their scalar gradients is one.
    ``more``: further scalar gradients behind the pair (DMoN's third loss)."""
    gs = (g_mc, g_o) + more
    if all(g is None for g in gs):
        return torch.zeros(len(gs), dtype=torch.float32, device=dev)
    z = None
    if any(g is None for g in gs):
        z = torch.zeros((), dtype=torch.float32, device=dev)
    return torch.stack([(g if g is not None else z).reshape(()) for g in gs])


# --------------------------------------------------------------------------- #
# DMoN pooling losses on the edge-list route
# --------------------------------------------------------------------------- #
DMON_STATS = 8     # floats per graph in hscn_dmon_sparse_fwd's statistics row (include/hscn.h)


class DMoNSparseFn(Function):
    """(logits, x) -> (S, spectral, ortho, cluster, pooled_x, pooled_adj): ``MinCutSparseFn``'s sibling for
    dense_dmon_pool (csrc/dmon.hip).  Gradients flow from the three losses to ``logits`` only."""

    @staticmethod
    def forward(ctx, logits: Tensor, x: Optional[Tensor], rel: Relation, node_ptr: Tensor, num_graphs: int):
        logits, x = _c(logits), _c(x)
        n, K = logits.shape
        dev = logits.device
        Fx = x.shape[1] if x is not None else 0
        S = torch.empty_like(logits)
        stats = torch.empty(num_graphs, DMON_STATS, dtype=torch.float32, device=dev)
        ss = torch.empty(num_graphs, K, K, dtype=torch.float32, device=dev)
        vec = torch.empty(num_graphs, 2, K, dtype=torch.float32, device=dev)
        px = torch.empty(num_graphs, K, max(Fx, 1), dtype=torch.float32, device=dev) if x is not None else None
        padj = torch.empty(num_graphs, K, K, dtype=torch.float32, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        row_csr = rel.csr_t  # keyed by edge ROW (= source side of edge_index)
        call("hscn_dmon_sparse_fwd", ptr(logits), ptr(x), ptr(row_csr.rowptr), ptr(row_csr.col), ptr(node_ptr),
             ptr(S), ptr(stats), ptr(ss), ptr(vec), ptr(px), ptr(padj), ptr(losses), n, num_graphs, K, Fx, stream())
        ctx.rel, ctx.G = rel, num_graphs
        ctx.save_for_backward(S, stats, ss, vec, node_ptr)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(S, padj)
        if px is not None:
            ctx.mark_non_differentiable(px)
        return S, losses[0], losses[1], losses[2], px, padj

    @staticmethod
    def backward(ctx, gS, g_sp, g_o, g_cl, g_px, g_padj):
        S, stats, ss, vec, node_ptr = ctx.saved_tensors
        rel: Relation = ctx.rel
        gl = _pack_loss_grads(g_sp, g_o, S.device, g_cl)
        g_logits = torch.empty_like(S)
        row_csr, col_csr = rel.csr_t, rel.csr
        call("hscn_dmon_sparse_bwd", ptr(S), ptr(stats), ptr(ss), ptr(vec), ptr(row_csr.rowptr), ptr(row_csr.col),
             ptr(col_csr.rowptr), ptr(col_csr.col), ptr(node_ptr), ptr(gl), ptr(g_logits), S.shape[0], ctx.G,
             S.shape[1], stream())
        return g_logits, None, None, None, None


# --------------------------------------------------------------------------- #
# MinCUT pooling, dense route (matrix cores)
# --------------------------------------------------------------------------- #
def _norm_ws(N: int, H: int, dev) -> Tensor:
    return torch.empty(max(1, _hip.lib().hscn_norm_workspace_bytes(N, H) // 4), dtype=torch.float32, device=dev)


class LayerNormFn(Function):
    """torch.nn.functional.layer_norm over the last dim of [N, H] (reference model/mpnn.py:55-56)."""

    @staticmethod
    def forward(ctx, x: Tensor, gamma: Tensor, beta: Tensor, eps: float):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        N, H = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(max(N, 1), dtype=torch.float32, device=x.device)
        rstd = torch.empty(max(N, 1), dtype=torch.float32, device=x.device)
        call("hscn_layer_norm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), N, H, float(eps), stream())
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, mean, rstd = ctx.saved_tensors
        N, H = x.shape
        gy = _c(gy)
        gx = torch.empty_like(x)
        gg = torch.empty(H, dtype=torch.float32, device=x.device)
        gb = torch.empty(H, dtype=torch.float32, device=x.device)
        ws = _norm_ws(N, H, x.device)
        call("hscn_layer_norm_bwd", ptr(gy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(gx), ptr(gg), ptr(gb), N, H,
             ptr(ws), ws.numel() * 4, stream())
        return gx, gg, gb, None


class BatchNormFn(Function):
    """torch.nn.functional.batch_norm on [N, H] (reference model/mpnn.py:53-54): batch statistics and the running
    update in training mode, running statistics in eval mode."""

    @staticmethod
    def forward(ctx, x: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor],
                running_var: Optional[Tensor], training: bool, momentum: float, eps: float):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        N, H = x.shape
        y = torch.empty_like(x)
        sm = torch.empty(H, dtype=torch.float32, device=x.device)
        sr = torch.empty(H, dtype=torch.float32, device=x.device)
        ws = _norm_ws(N, H, x.device)
        call("hscn_batch_norm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(y), ptr(sm),
             ptr(sr), N, H, float(eps), float(momentum), 1 if training else 0, ptr(ws), ws.numel() * 4, stream())
        ctx.save_for_backward(x, gamma, sm, sr)
        ctx.training = bool(training)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, sm, sr = ctx.saved_tensors
        N, H = x.shape
        gy = _c(gy)
        gx = torch.empty_like(x)
        gg = torch.empty(H, dtype=torch.float32, device=x.device)
        gb = torch.empty(H, dtype=torch.float32, device=x.device)
        ws = _norm_ws(N, H, x.device)
        call("hscn_batch_norm_bwd", ptr(gy), ptr(x), ptr(gamma), ptr(sm), ptr(sr), ptr(gx), ptr(gg), ptr(gb), N, H,
             1 if ctx.training else 0, ptr(ws), ws.numel() * 4, stream())
        return gx, gg, gb, None, None, None, None, None


class MinCutDenseRaggedFn(Function):
    """``MinCutDenseFn`` for a batch of graphs of DIFFERENT sizes: (logits [N,K], x [N,F] | None, adj [B,nmax,nmax]
    float32 -- or uint8 [B,nmax,round_up(nmax,32)] -- zero beyond each graph, nptr int32 [B+1], gid int32 [N]) -> (S [N,K], mincut, ortho, pooled_x, pooled_adj);
    losses = mean over graphs, every graph's terms equal to the single-graph call's (hscn_mincut_dense_ragged_*)."""

    @staticmethod
    def forward(ctx, logits: Tensor, x: Optional[Tensor], adj: Tensor, nptr: Tensor, gid: Tensor,
                asym: Optional[Tensor] = None):
        """asym (uint8 adjacency only): int32 [B] from ``to_dense_adj_ragged(..., symmetry=True)`` -- graphs flagged 0 are
        symmetric, and the backward takes their ``A^T S`` from the forward's ``A S`` instead of computing it."""
        if adj.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"the dense adjacency is float32 or uint8 (got {adj.dtype})")
        logits, x, adj = _c(logits), _c(x), adj.contiguous()
        N, K = logits.shape
        B, nmax = adj.shape[0], adj.shape[1]
        dev = logits.device
        Fx = x.shape[1] if x is not None else 0
        S = torch.empty_like(logits)
        AS = torch.empty_like(logits)
        deg = torch.empty(N, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
        ss = torch.empty(B, K, K, dtype=torch.float32, device=dev)
        px = torch.empty(B, K, Fx, dtype=torch.float32, device=dev) if x is not None else None
        padj = torch.empty(B, K, K, dtype=torch.float32, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        call("hscn_mincut_dense_ragged_fwd", ptr(x), ptr(adj), adj.element_size(), ptr(logits), ptr(nptr), N, B, nmax, K, Fx, ptr(S), ptr(AS),
             ptr(deg), ptr(stats), ptr(ss), ptr(px), ptr(padj), ptr(losses), stream())
        ctx.has_asym = asym is not None and adj.dtype == torch.uint8
        if ctx.has_asym:
            ctx.save_for_backward(adj, S, AS, deg, stats, ss, nptr, gid, asym)
        else:
            ctx.save_for_backward(adj, S, AS, deg, stats, ss, nptr, gid)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(S, padj)
        if px is not None:
            ctx.mark_non_differentiable(px)
        return S, losses[0], losses[1], px, padj

    @staticmethod
    def backward(ctx, gS, g_mc, g_o, g_px, g_padj):
        if ctx.has_asym:
            adj, S, AS, deg, stats, ss, nptr, gid, asym = ctx.saved_tensors
        else:
            adj, S, AS, deg, stats, ss, nptr, gid = ctx.saved_tensors
            asym = None
        N, K = S.shape
        B, nmax = adj.shape[0], adj.shape[1]
        gl = _pack_loss_grads(g_mc, g_o, S.device)
        AtS = torch.empty_like(S)
        SG = torch.empty_like(S)
        Gss = torch.empty_like(ss)
        g_logits = torch.empty_like(S)
        call("hscn_mincut_dense_ragged_bwd_sym", ptr(adj), adj.element_size(), ptr(S), ptr(AS), ptr(deg), ptr(stats), ptr(ss), ptr(gl),
             ptr(nptr), ptr(gid), N, B, nmax, K, ptr(AtS), ptr(SG), ptr(Gss), ptr(g_logits), ptr(asym), stream())
        return g_logits, None, None, None, None, None


class MinCutDenseFn(Function):
    """(logits [B,n,K], x [B,n,F] | None, adj [B,n,n]) -> (S, mincut, ortho, pooled_x, pooled_adj).
    Gradients flow from the two losses to ``logits``."""

    @staticmethod
    def forward(ctx, logits: Tensor, x: Optional[Tensor], adj: Tensor):
        logits, x, adj = _c(logits), _c(x), _c(adj)
        B, n, K = logits.shape
        dev = logits.device
        Fx = x.shape[2] if x is not None else 0
        S = torch.empty_like(logits)
        AS = torch.empty_like(logits)
        deg = torch.empty(B, n, dtype=torch.float32, device=dev)
        stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
        ss = torch.empty(B, K, K, dtype=torch.float32, device=dev)
        px = torch.empty(B, K, Fx, dtype=torch.float32, device=dev) if x is not None else None
        padj = torch.empty(B, K, K, dtype=torch.float32, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        call("hscn_mincut_dense_fwd", ptr(x), ptr(adj), ptr(logits), B, n, K, Fx, ptr(S), ptr(AS), ptr(deg),
             ptr(stats), ptr(ss), ptr(px), ptr(padj), ptr(losses), stream())
        ctx.save_for_backward(adj, S, AS, deg, stats, ss)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(S, padj)
        if px is not None:
            ctx.mark_non_differentiable(px)
        return S, losses[0], losses[1], px, padj

    @staticmethod
    def backward(ctx, gS, g_mc, g_o, g_px, g_padj):
        adj, S, AS, deg, stats, ss = ctx.saved_tensors
        B, n, K = S.shape
        gl = _pack_loss_grads(g_mc, g_o, S.device)
        AtS = torch.empty_like(S)
        SG = torch.empty_like(S)
        Gss = torch.empty_like(ss)
        g_logits = torch.empty_like(S)
        call("hscn_mincut_dense_bwd", ptr(adj), ptr(S), ptr(AS), ptr(deg), ptr(stats), ptr(ss), ptr(gl), B, n, K,
             ptr(AtS), ptr(SG), ptr(Gss), ptr(g_logits), stream())
        return g_logits, None, None
