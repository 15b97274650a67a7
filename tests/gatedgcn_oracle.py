"""Plain-torch restatement of GatedGCN (GraphGPS's GatedGCNLayer; residual gated graph ConvNets), written from the
formulas (CPU, any float dtype).  With j = edge_index[0, k] the source and i = edge_index[1, k] the target of edge k:

    e^_k  = Dx_i + Ex_j + Ce_k                                 the layer's new edge features (pre-norm), row k = edge k
    s_k   = sigmoid(e^_k)
    num_i = sum_{k: dst_k = i} s_k * Bx_j      den_i = sum_{k: dst_k = i} s_k
    h_i   = Ax_i + num_i / (den_i + 1e-6)

every edge as given: loops and repeated edges count.  The float32 and float64 evaluations of these modules are the two
oracles of tests/test_gpu_gatedgcn.py; ``skip`` removes one edge from both sums (the toothed variant; its row of e^ stays).
``watch(tag, tensor)`` receives every ReLU input for the kink guard -- the gate itself is smooth, so only the ReLUs after
the layers, in the feed-forward blocks and in the heads have kinks."""
import torch
import torch.nn as nn

from tests import gps_oracle as GP

EPS = 1e-6


def edge_pre(Dx, Ex, Ce, edge_index):
    """e^ [E, H]."""
    return Dx[edge_index[1]] + Ex[edge_index[0]] + Ce


def sums(Bx, e_hat, edge_index, skip=None):
    """(num, den) [N, H] each; ``skip``: an edge number left out of both."""
    src, dst = edge_index[0], edge_index[1]
    s = torch.sigmoid(e_hat)
    m = s * Bx[src]
    if skip is not None:
        keep = torch.ones(e_hat.size(0), dtype=torch.bool)
        keep[skip] = False
        s, m, dst = s[keep], m[keep], dst[keep]
    num = torch.zeros_like(Bx).index_add_(0, dst, m)
    den = torch.zeros_like(Bx).index_add_(0, dst, s)
    return num, den


def aggregate(Ax, Bx, Dx, Ex, Ce, edge_index, skip=None):
    """(h [N, H], e^ [E, H])."""
    e_hat = edge_pre(Dx, Ex, Ce, edge_index)
    num, den = sums(Bx, e_hat, edge_index, skip)
    return Ax + num / (den + EPS), e_hat


def magnitudes(Ax, Bx, Dx, Ex, Ce, edge_index):
    """The same sums over absolute values, for the a-priori bound: {"e": |Dx_i| + |Ex_j| + |Ce_k| [E, H],
    "num": sum_k s_k |Bx_j|, "den": sum_k s_k, "dsum": sum_k mag_e_k, "dsumB": sum_k mag_e_k |Bx_j| (all [N, H]),
    "deg": in-degree [N, 1]}."""
    src, dst = edge_index[0], edge_index[1]
    mag_e = Dx.abs()[dst] + Ex.abs()[src] + Ce.abs()
    s = torch.sigmoid(edge_pre(Dx, Ex, Ce, edge_index))
    z = torch.zeros_like(Bx)
    return {"e": mag_e,
            "num": z.clone().index_add_(0, dst, s * Bx.abs()[src]),
            "den": z.clone().index_add_(0, dst, s),
            "dsum": z.clone().index_add_(0, dst, mag_e),              # sum_k mag_e_k: the gates' input error, summed
            "dsumB": z.clone().index_add_(0, dst, mag_e * Bx.abs()[src]),
            "deg": torch.bincount(dst, minlength=Bx.size(0)).to(Bx.dtype).unsqueeze(1)}


def backward_by_hand(Ax, Bx, Dx, Ex, Ce, edge_index, gh, ge_hat=None):
    """The backward formulas the kernels implement, evaluated with torch ops: {Ax, Bx, Dx, Ex, Ce: gradient}."""
    src, dst = edge_index[0], edge_index[1]
    h, e_hat = aggregate(Ax, Bx, Dx, Ex, Ce, edge_index)
    _, den = sums(Bx, e_hat, edge_index)
    s = torch.sigmoid(e_hat)
    gn = gh / (den + EPS)
    gd = -gn * (h - Ax)
    ge = (gn[dst] * Bx[src] + gd[dst]) * s * (1 - s)
    if ge_hat is not None:
        ge = ge_hat + ge
    z = torch.zeros_like(Ax)
    return {"Ax": gh, "Bx": z.clone().index_add_(0, src, s * gn[dst]), "Dx": z.clone().index_add_(0, dst, ge),
            "Ex": z.clone().index_add_(0, src, ge), "Ce": ge}


class GatedGCNConvRef(nn.Module):
    """Five ``torch.nn.Linear`` under GraphGPS's names; returns (x_out, e_out), ``act`` ("relu" / "identity") on both."""

    def __init__(self, in_channels, out_channels, edge_dim):
        super().__init__()
        self.A = nn.Linear(in_channels, out_channels)
        self.B = nn.Linear(in_channels, out_channels)
        self.C = nn.Linear(edge_dim, out_channels)
        self.D = nn.Linear(in_channels, out_channels)
        self.E = nn.Linear(in_channels, out_channels)
        self.watch = None

    def aggregate(self, x, edge_index, edge_attr, skip=None):
        return aggregate(self.A(x), self.B(x), self.D(x), self.E(x), self.C(edge_attr), edge_index, skip)

    def forward(self, x, edge_index, edge_attr, act="identity", skip=None):
        h, e = self.aggregate(x, edge_index, edge_attr, skip)
        if act == "relu":
            if self.watch is not None:
                self.watch("node output", h)
                self.watch("edge output", e)
            h, e = torch.relu(h), torch.relu(e)
        return h, e


class GatedGCNLayerRef(GatedGCNConvRef):
    """GraphGPS's layer: conv, batch norm on x and e, ReLU, dropout (masks given by the caller), residuals."""

    def __init__(self, channels, residual=True, norm="batch", edge_dim=None):
        super().__init__(channels, channels, channels if edge_dim is None else edge_dim)
        self.channels, self.residual = channels, residual
        self.bn_node_x = GP._norm(norm, channels)
        self.bn_edge_e = GP._norm(norm, channels)

    def forward(self, x, edge_index, edge_attr, skip=None, masks=None):
        """``masks = (node mask [N, D], edge mask [E, D])``: dropout's keep masks, already scaled by 1 / (1 - p)."""
        h, e = self.aggregate(x, edge_index, edge_attr, skip)
        if self.bn_node_x is not None:
            h, e = self.bn_node_x(h), self.bn_edge_e(e)
        if self.watch is not None:
            self.watch("node ReLU input", h)
            self.watch("edge ReLU input", e)
        h, e = torch.relu(h), torch.relu(e)
        if masks is not None:
            h, e = h * masks[0], e * masks[1]
        if self.residual:
            h = x + h
            if edge_attr.size(-1) == self.channels:
                e = edge_attr + e
        return h, e


class GatedGCNModelRef(nn.Module):
    """The MPNN baseline with conv = GatedGCNConv: L layers F -> H -> ... -> C, ReLU on both outputs of every hidden
    layer, e carried forward (C_0: De -> H, C_l: H -> H, the last H -> C), the last layer's edge output dropped; then
    the per-graph mean ("graph"), the node outputs ("node") or the dot product of candidate pairs ("link")."""

    def __init__(self, F, H, C, L, edge_dim, task_level="graph"):
        super().__init__()
        dims = [(F, H, edge_dim)] + [(H, H, H)] * (L - 2) + [(H, C, H)]
        self.conv_layers = nn.ModuleList(GatedGCNConvRef(i, o, d) for i, o, d in dims)
        self.task_level = task_level

    def set_watch(self, watch):
        for i, c in enumerate(self.conv_layers):
            c.watch = None if watch is None else (lambda tag, t, i=i: watch(f"layer {i} {tag}", t))

    def forward(self, x, edge_index, edge_attr, batch, num_graphs, pairs=None, skip=None):
        e = edge_attr
        for c in self.conv_layers[:-1]:
            x, e = c(x, edge_index, e, "relu", skip)
        x, _ = self.conv_layers[-1](x, edge_index, e, "identity", skip)
        if self.task_level == "node":
            return x
        if self.task_level == "link":
            return (x[pairs[0]] * x[pairs[1]]).sum(1)
        sums_ = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
        return sums_ / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)


class GatedGPSLayerRef(GP.GPSLayerRef):
    """``GPSLayerRef`` with the gated local branch: h_l = norm1_local(GatedGCNLayer(x, e)) -- no second dropout or
    residual around it -- and the layer's new edge features returned beside h."""

    def __init__(self, D, heads, norm="layer"):
        super().__init__(D, None, heads, norm)
        self.local_conv = "gatedgcn"
        self.conv = GatedGCNLayerRef(D, residual=True, norm="batch")
        self.norm1_local = GP._norm(norm, D)

    def set_watch(self, watch, prefix=""):
        self.watch = None if watch is None else (lambda tag, t: watch(prefix + tag, t))
        self.conv.watch = self.watch

    def forward(self, x, edge_index, ptr, edge_attr=None, skip=None, att_skip=None):
        """``skip``: an EDGE number left out of the gated sums; ``att_skip = (g, j)``: key j of graph g left out of
        the attention (``GPSLayerRef``'s toothed variant)."""
        h_a = x + self.attn(x, ptr, att_skip)
        if self.norm1_attn is not None:
            h_a = self.norm1_attn(h_a)
        h_l, e = self.conv(x, edge_index, edge_attr, skip)
        if self.norm1_local is not None:
            h_l = self.norm1_local(h_l)
        h = h_l + h_a
        f = self.ff_linear1(h)
        if self.watch is not None:
            self.watch("feed-forward hidden layer", f)
        h = h + self.ff_linear2(torch.relu(f))
        if self.norm2 is not None:
            h = self.norm2(h)
        return h, e


class GatedGPSRef(GP.GPSRef):
    """``GPSRef`` with ``local_conv="gatedgcn"``: ``edge_encoder`` in front, edge features handed from layer to layer."""

    def __init__(self, F, D, C, L, heads, edge_dim, norm="layer", task_level="graph"):
        super().__init__(F, D, C, 0, heads, None, norm, task_level)
        self.layers = nn.ModuleList(GatedGPSLayerRef(D, heads, norm) for _ in range(L))
        self.edge_encoder = nn.Linear(edge_dim, D)

    def forward(self, x, edge_index, edge_attr, batch, ptr, num_graphs, pairs=None, skip=None, att_skip=None,
                pool_skip=None):
        """``skip``: an edge left out of every layer's gated sums; ``att_skip`` / ``pool_skip``: as ``GPSRef``."""
        x = self.node_encoder(x)
        e = self.edge_encoder(edge_attr)
        for layer in self.layers:
            x, e = layer(x, edge_index, ptr, e, skip, att_skip)
        if self.task_level == "graph":
            if pool_skip is not None:
                keep = torch.ones(x.size(0), 1, dtype=x.dtype)
                keep[pool_skip] = 0
                x = x * keep
            s = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
            x = s / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)
        h = self.lin_1(x)
        if self.watch is not None:
            self.watch("head hidden layer", h)
        out = self.lin_2(torch.relu(h))
        if self.task_level == "link":
            return (out[pairs[0]] * out[pairs[1]]).sum(1)
        return out
