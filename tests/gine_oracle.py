"""Plain-torch restatement of GINEConv with edge features, written from the formula (CPU, any float dtype):

    m_k = relu(x[src_k] + lin(edge_attr[k]))          lin: Linear(edge_dim, F) with bias
    z_i = (1 + eps) * x_i + sum_{k: dst_k = i} m_k    every edge as given: loops and repeated edges count
    out = nn(z)

The float32 and float64 evaluations of these modules are the two oracles of tests/test_gpu_gine.py; ``skip`` removes
one edge (the toothed variant).  ``watch(tag, tensor)`` receives every ReLU input (the messages' pre-activations, the
MLP's hidden layer, the ReLU between the model's layers) for the kink guard."""
import torch
import torch.nn as nn


def pre_activations(x, edge_index, edge_attr, W, b):
    """[E, F]: x[src_k] + W e_k + b."""
    return x[edge_index[0]] + edge_attr @ W.t() + b


def aggregate(x, edge_index, edge_attr, W, b, eps=0.0, skip=None, watch=None):
    """z [N, F]; ``skip``: an edge number left out of the sum."""
    pre = pre_activations(x, edge_index, edge_attr, W, b)
    dst = edge_index[1]
    if skip is not None:
        keep = torch.ones(pre.size(0), dtype=torch.bool)
        keep[skip] = False
        pre, dst = pre[keep], dst[keep]
    if watch is not None:
        watch("message pre-activation", pre)
    return torch.zeros_like(x).index_add_(0, dst, torch.relu(pre)) + (1.0 + eps) * x


def aggregate_magnitude(x, edge_index, edge_attr, W, b, eps=0.0):
    """The same sum over absolute values: (1+eps)|x_i| + sum_k (|x_src| + |W||e_k| + |b|), and the per-row length
    n_i = deg_i + De + 4 of the sums behind an element (helpers.f64_close)."""
    mag_pre = pre_activations(x.abs(), edge_index, edge_attr.abs(), W.abs(), b.abs())
    mag = torch.zeros_like(x).index_add_(0, edge_index[1], mag_pre) + (1.0 + abs(eps)) * x.abs()
    deg = torch.bincount(edge_index[1], minlength=x.size(0)).to(torch.float64)
    return mag, (deg + edge_attr.size(1) + 4).unsqueeze(1)


class GINEConvRef(nn.Module):
    """``nn`` is a torch module; ``lin`` a ``torch.nn.Linear(edge_dim, F)``; ``eps`` a buffer: PyG's names."""

    def __init__(self, mlp, edge_dim, in_channels, eps=0.0):
        super().__init__()
        self.nn = mlp
        self.lin = nn.Linear(edge_dim, in_channels)
        self.register_buffer("eps", torch.tensor([float(eps)]))
        self.watch = None

    def forward(self, x, edge_index, edge_attr, skip=None):
        z = aggregate(x, edge_index, edge_attr, self.lin.weight, self.lin.bias, float(self.eps), skip, self.watch)
        if self.watch is not None and isinstance(self.nn, nn.Sequential):
            h = self.nn[0](z)
            self.watch("MLP hidden layer", h)
            for m in list(self.nn)[1:]:
                h = m(h)
            return h
        return self.nn(z)


def gine_layer(in_channels, out_channels, edge_dim, eps=0.0):
    """GraphGPS's GINE layer: GINEConv over Linear - ReLU - Linear."""
    return GINEConvRef(nn.Sequential(nn.Linear(in_channels, out_channels), nn.ReLU(),
                                     nn.Linear(out_channels, out_channels)), edge_dim, in_channels, eps)


class GINEModelRef(nn.Module):
    """The MPNN baseline with conv = GINE: L layers F -> H -> ... -> C with a ReLU after each hidden one, then the
    per-graph mean ("graph"), the node outputs ("node") or the dot product of candidate pairs ("link")."""

    def __init__(self, F, H, C, L, edge_dim, task_level="graph"):
        super().__init__()
        dims = [(F, H)] + [(H, H)] * (L - 2) + [(H, C)]
        self.conv_layers = nn.ModuleList(gine_layer(i, o, edge_dim) for i, o in dims)
        self.task_level = task_level
        self.watch = None

    def set_watch(self, watch):
        self.watch = watch
        for i, c in enumerate(self.conv_layers):
            c.watch = None if watch is None else (lambda tag, t, i=i: watch(f"layer {i} {tag}", t))

    def forward(self, x, edge_index, edge_attr, batch, num_graphs, skip=None):
        for i, c in enumerate(self.conv_layers[:-1]):
            x = c(x, edge_index, edge_attr, skip)
            if self.watch is not None:
                self.watch(f"layer {i} output", x)
            x = torch.relu(x)
        x = self.conv_layers[-1](x, edge_index, edge_attr, skip)
        if self.task_level != "graph":
            return x
        sums = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
        return sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)


def copy_weights(ref, product):
    """The restatement's weights into the product module (same names: nn.*, lin.*, eps)."""
    sd = {k: v.detach().clone().float() for k, v in ref.state_dict().items()}
    missing = product.load_state_dict(sd, strict=True)
    return missing
