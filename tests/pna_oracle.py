"""Plain-torch restatement of PNAConv (PyG, towers = 1, one pre and one post Linear), written from the formulas (CPU,
any float dtype):

    m_k   = pre_nn(cat[x_dst, x_src, edge_encoder(e_k)])           (operator level: m_k = a[dst_k] + b[src_k] + t_k)
    mean, min, max, sum over {k: dst_k = i};  std = sqrt(relu(mean(m^2) - mean(m)^2) + 1e-5)
    a node without in-edges: 0 for mean, min, max, sum and sqrt(1e-5) for std
    scalers with d = max(deg_i, 1): identity 1, amplification log(d + 1) / avg_deg_log, attenuation its inverse
    columns: scaler-major, then aggregator-major, then F
    out   = lin(post_nn(cat[x_i, aggregated_i]))

min and max select their edge EXPLICITLY by the library's rule -- the first in-edge of the node, in the order of the
edge list, that attains the extreme -- and gather ``m`` there, so that autograd sends the whole gradient to that edge
(torch's ``scatter_reduce`` would split it evenly among tied edges).  ``skip`` removes one edge (the toothed variant).
The float32 and float64 evaluations are the two oracles of tests/test_gpu_pna.py; this file is the definition the
feature is held to."""
import torch
import torch.nn as nn

AGGREGATORS = ("mean", "min", "max", "sum", "std")
SCALERS = ("identity", "amplification", "attenuation")
STD_EPS = 1e-5


def first_extreme(m, dst, N, largest):
    """[N, F] int64: per (node, column) the number of the FIRST edge into the node whose message attains the max
    (``largest``) or the min; E for a node without in-edges.  Computed on detached values: a selection, no gradient."""
    E, F = m.shape
    v = m.detach()
    idx = dst.unsqueeze(1).expand(E, F)
    fill = float("-inf") if largest else float("inf")
    ext = torch.full((N, F), fill, dtype=v.dtype).scatter_reduce(0, idx, v, "amax" if largest else "amin",
                                                                   include_self=True)
    hit = v == ext[dst]
    cand = torch.where(hit, torch.arange(E).unsqueeze(1).expand(E, F), torch.full((E, F), E))
    return torch.full((N, F), E, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin", include_self=True)


def aggregate_messages(m, dst, N, aggregators, scalers, avg_deg_log=None):
    """[N, S A F] from the messages m [E, F] and their targets dst [E]."""
    E, F = m.shape
    deg = torch.bincount(dst, minlength=N)
    cnt = deg.clamp(min=1).to(m.dtype).unsqueeze(1)
    total = torch.zeros(N, F, dtype=m.dtype).index_add_(0, dst, m)
    mean = total / cnt
    padded = torch.cat([m, torch.zeros(1, F, dtype=m.dtype)], 0)           # row E: what an empty node gathers
    outs = []
    for name in aggregators:
        if name == "mean":
            outs.append(mean)
        elif name == "sum":
            outs.append(total)
        elif name in ("min", "max"):
            outs.append(padded.gather(0, first_extreme(m, dst, N, name == "max")))
        elif name == "std":
            mean_sq = torch.zeros(N, F, dtype=m.dtype).index_add_(0, dst, m * m) / cnt
            outs.append(torch.sqrt(torch.relu(mean_sq - mean * mean) + STD_EPS))
        else:
            raise ValueError(name)
    block = torch.cat(outs, 1)
    d = deg.clamp(min=1).to(m.dtype).unsqueeze(1)
    scaled = []
    for name in scalers:
        if name == "identity":
            scaled.append(block)
        elif name == "amplification":
            scaled.append(block * (torch.log(d + 1) / avg_deg_log))
        elif name == "attenuation":
            scaled.append(block * (avg_deg_log / torch.log(d + 1)))
        else:
            raise ValueError(name)
    return torch.cat(scaled, 1)


def _without(edge_index, rows, skip):
    if skip is None:
        return edge_index, rows
    keep = torch.ones(edge_index.size(1), dtype=torch.bool)
    keep[skip] = False
    return edge_index[:, keep], [None if r is None else r[keep] for r in rows]


def messages(a, b, t, edge_index):
    """[E, F]: a[dst_k] + b[src_k] + t_k."""
    m = a[edge_index[1]] + b[edge_index[0]]
    return m if t is None else m + t


def aggregate(a, b, t, edge_index, aggregators, scalers, avg_deg_log=None, skip=None):
    """The operator: (a [N, F], b [N, F], t [E, F] or None) -> [N, S A F]; ``skip``: an edge number left out."""
    ei, (t,) = _without(edge_index, [t], skip)
    return aggregate_messages(messages(a, b, t, ei), ei[1], a.size(0), aggregators, scalers, avg_deg_log)


class PNAConvRef(nn.Module):
    """PyG's parameter names: pre_nns.0.0, post_nns.0.0, lin, edge_encoder (only with ``edge_dim``)."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, avg_deg_log=None, edge_dim=None):
        super().__init__()
        F = in_channels
        self.aggregators, self.scalers, self.avg_deg_log = tuple(aggregators), tuple(scalers), avg_deg_log
        self.edge_encoder = nn.Linear(edge_dim, F) if edge_dim is not None else None
        self.pre_nns = nn.ModuleList([nn.Sequential(nn.Linear((3 if edge_dim is not None else 2) * F, F))])
        self.post_nns = nn.ModuleList([nn.Sequential(nn.Linear((len(aggregators) * len(scalers) + 1) * F, out_channels))])
        self.lin = nn.Linear(out_channels, out_channels)

    def forward(self, x, edge_index, edge_attr=None, skip=None):
        ei, (ea,) = _without(edge_index, [edge_attr], skip)
        parts = [x[ei[1]], x[ei[0]]]
        if self.edge_encoder is not None:
            parts.append(self.edge_encoder(ea))
        m = self.pre_nns[0](torch.cat(parts, 1))
        agg = aggregate_messages(m, ei[1], x.size(0), self.aggregators, self.scalers, self.avg_deg_log)
        return self.lin(self.post_nns[0](torch.cat([x, agg], 1)))


DEFAULT_AGGREGATORS = ("mean", "min", "max", "std")
DEFAULT_SCALERS = ("identity",)


class PNAModelRef(nn.Module):
    """The MPNN baseline with conv = PNA / PNAEdge: L layers F -> H -> ... -> C with a ReLU after each hidden one, then
    the per-graph mean ("graph"), the node outputs ("node") or the dot product of candidate pairs ("link")."""

    def __init__(self, F, H, C, L, edge_dim=None, task_level="graph", aggregators=DEFAULT_AGGREGATORS,
                 scalers=DEFAULT_SCALERS, avg_deg_log=None):
        super().__init__()
        dims = [(F, H)] + [(H, H)] * (L - 2) + [(H, C)]
        self.conv_layers = nn.ModuleList(PNAConvRef(i, o, aggregators, scalers, avg_deg_log, edge_dim) for i, o in dims)
        self.task_level = task_level
        self.watch = None

    def forward(self, x, edge_index, edge_attr, batch, num_graphs, pairs=None, skip=None):
        for i, c in enumerate(self.conv_layers[:-1]):
            x = c(x, edge_index, edge_attr, skip)
            if self.watch is not None:
                self.watch(f"layer {i} output", x)
            x = torch.relu(x)
        x = self.conv_layers[-1](x, edge_index, edge_attr, skip)
        if self.task_level == "node":
            return x
        if self.task_level == "link":
            return (x[pairs[0]] * x[pairs[1]]).sum(1)
        sums = torch.zeros(num_graphs, x.size(1), dtype=x.dtype).index_add_(0, batch, x)
        return sums / torch.bincount(batch, minlength=num_graphs).clamp(min=1).to(x.dtype).unsqueeze(1)
