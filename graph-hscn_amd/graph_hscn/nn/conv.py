"""Message-passing modules with the torch_geometric signatures, parameter names
and initialisers the reference relies on (model/hscn.py:6-14,83-96,117-125;
config/config.py:19-23), computing through the HIP kernels.

``state_dict`` keys match PyG 2.2/2.3 so checkpoints move
between the reference and this package unchanged.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from .._hip import ACT
from ..structure import Relation, relation_of, self_loop_relation_of
from . import functional as Fh


def _glorot(t: Tensor) -> Tensor:
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        return t.uniform_(-a, a)


class Linear(nn.Module):
    """torch_geometric.nn.Linear: ``y = x W^T + b``; 'glorot' or kaiming-uniform
    (a=sqrt 5) weights; ``in_channels=-1`` is materialised on first use."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True,
                 weight_initializer: Optional[str] = None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight_initializer = weight_initializer
        if in_channels > 0:
            self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        else:
            self.weight = nn.parameter.UninitializedParameter()
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self) -> None:
        if self.in_channels <= 0:
            return
        if self.weight_initializer == "glorot":
            _glorot(self.weight)
        else:
            nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels)
            nn.init.uniform_(self.bias, -bound, bound)

    def materialize(self, in_channels: int, like: Tensor) -> None:
        if isinstance(self.weight, nn.parameter.UninitializedParameter):
            self.in_channels = int(in_channels)
            self.weight.materialize((self.out_channels, self.in_channels), device=like.device,
                                    dtype=torch.float32)
            self.reset_parameters()

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        # as torch_geometric.nn.Linear: a weight that is not materialised yet is listed as it is (it cannot be detached)
        if isinstance(self.weight, nn.parameter.UninitializedParameter):
            destination[prefix + "weight"] = self.weight
            if self.bias is not None:
                destination[prefix + "bias"] = self.bias if keep_vars else self.bias.detach()
            return
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def forward(self, x: Tensor, act: str = "identity") -> Tensor:
        self.materialize(x.size(-1), x)
        return Fh.linear(x, self.weight, self.bias, act)


def _relation(edge_index: Union[Tensor, Relation], num_src: int, num_dst: int, both: bool = False) -> Relation:
    if isinstance(edge_index, Relation):
        return edge_index
    return relation_of(edge_index, num_src, num_dst, both=both)


class GraphConv(nn.Module):
    """PyG GraphConv(aggr='add'): ``lin_rel(sum_j w_ji x_j) + lin_root(x_i)``
    (used at model/hscn.py:32,40)."""

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "add", bias: bool = True):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError("GraphConv on the hot path uses aggr='add'")
        self.lin_rel = Linear(in_channels, out_channels, bias=bias)
        self.lin_root = Linear(in_channels, out_channels, bias=False)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_weight: Optional[Tensor] = None,
                act: str = "identity") -> Tensor:
        # (sum_j w_ji x_j) W_rel + x W_root: only a gradient w.r.t. x walks the source-keyed CSR
        rel = _relation(edge_index, x.size(0), x.size(0), both=torch.is_grad_enabled() and x.requires_grad)
        return Fh.GraphConvFn.apply(x, edge_weight, self.lin_rel.weight, self.lin_rel.bias,
                                    self.lin_root.weight, rel, ACT[act])


class GCNConv(nn.Module):
    """PyG GCNConv, ``normalize=True``, unit edge weights.
    ``add_self_loops=False`` is what build_conv_relation constructs (model/hscn.py:117-125);
    the default ``add_self_loops=True`` is what the MPNN baseline constructs (model/mpnn.py:28-32):
    the same kernels over the edge list with one loop per node appended, whose in-degree is
    gcn_norm's degree."""

    def __init__(self, in_channels: int, out_channels: int, add_self_loops: bool = True,
                 cached: bool = False, bias: bool = True):
        super().__init__()
        self.add_self_loops = bool(add_self_loops)
        self.lin = Linear(in_channels, out_channels, bias=False, weight_initializer="glorot")
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], act: str = "identity") -> Tensor:
        self.lin.materialize(x.size(-1), x)
        if isinstance(edge_index, Relation):
            rel = edge_index                      # the caller built the structure (loops included if wanted)
        else:
            # A_hat (X W): with gradients on, the backward walks the source-keyed CSR for the weight gradient already
            both = torch.is_grad_enabled()
            if self.add_self_loops:
                rel = self_loop_relation_of(edge_index, x.size(0), both=both)
            else:
                rel = relation_of(edge_index, x.size(0), x.size(0), both=both)
        return Fh.GCNConvFn.apply(x, self.lin.weight, self.bias, rel, ACT[act])


class GCN2Conv(nn.Module):
    """PyG GCN2Conv (GCNII; Chen et al. 2020), ``add_self_loops=True``, ``normalize=True``, unit edge weights:

        p   = A_hat x                                    A_hat: GCNConv's symmetric normalisation with self loops
        out = (1 - beta) h + beta h weight1,             h = (1 - alpha) p + alpha x_0               (shared_weights)
        out = (1 - beta) h + beta ((1 - alpha) p weight1 + alpha x_0 weight2)                        (otherwise)

    ``beta = log(theta / layer + 1)``, or 1 when ``theta`` or ``layer`` is None.  Parameters and ``state_dict`` keys
    are PyG's: ``weight1`` [channels, channels] and, with ``shared_weights=False``, ``weight2``; glorot; no bias.
    ``forward(x, x_0, edge_index_or_Relation, act=...)``: ``x_0`` may be longer than ``x`` (its first N rows are read, as
    PyG slices them); a ``Relation`` is the self-loop relation already built (``structure.self_loop_relation_of``),
    which a model's layers share.  The layer is ONE launch (csrc/gcn2.hip), ``act`` ("identity" or "relu") applied in
    its epilogue.

    Not provided, refused by name: ``edge_weight=``, ``cached=True``, ``normalize=False``, ``add_self_loops=False``."""

    def __init__(self, channels: int, alpha: float, theta: Optional[float] = None, layer: Optional[int] = None,
                 shared_weights: bool = True, cached: bool = False, add_self_loops: bool = True,
                 normalize: bool = True):
        super().__init__()
        if cached:
            raise NotImplementedError("GCN2Conv(cached=True): the normalised structure is cached per edge_index tensor "
                                      "already (structure.self_loop_relation_of); cached must be False")
        if not normalize:
            raise NotImplementedError("GCN2Conv(normalize=False): the operator applies GCNConv's symmetric "
                                      "normalisation; an unnormalised propagation is not provided")
        if not add_self_loops:
            raise NotImplementedError("GCN2Conv(add_self_loops=False): the operator runs over the relation with one "
                                      "loop per node, as GCNConv(add_self_loops=True) builds it")
        channels = int(channels)
        if not Fh.gcn2_supported(channels):
            raise ValueError(f"GCN2Conv: channels = {channels} outside the kernel's envelope ({Fh.GCN2_ENVELOPE})")
        if (theta is not None and not float(theta) > 0.0) or (layer is not None and int(layer) < 1):
            raise ValueError(f"GCN2Conv: theta must be positive and layer >= 1 (or None), got {theta!r}, {layer!r}")
        self.channels, self.theta, self.layer = channels, theta, layer
        self.beta = 1.0 if theta is None or layer is None else math.log(float(theta) / int(layer) + 1.0)
        self.alpha, self.beta = Fh._check_gcn2_coeffs(alpha, self.beta)
        self.shared_weights = bool(shared_weights)
        self.weight1 = nn.Parameter(torch.empty(channels, channels))
        if self.shared_weights:
            self.register_parameter("weight2", None)
        else:
            self.weight2 = nn.Parameter(torch.empty(channels, channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _glorot(self.weight1)
        if self.weight2 is not None:
            _glorot(self.weight2)

    def forward(self, x: Tensor, x_0: Tensor, edge_index: Union[Tensor, Relation], edge_weight: Optional[Tensor] = None,
                act: str = "identity") -> Tensor:
        if edge_weight is not None:
            raise NotImplementedError("GCN2Conv(edge_weight=...): the operator propagates unit edge weights; "
                                      "edge_weight must be None")
        if act not in Fh.GCN2_ACTS:
            raise ValueError(f"GCN2Conv: act must be one of {Fh.GCN2_ACTS}, got {act!r}")
        if not isinstance(x, Tensor) or x.dim() != 2 or x.size(1) != self.channels:
            raise ValueError(f"GCN2Conv: x must be [N, {self.channels}], got {tuple(getattr(x, 'shape', ()))}")
        n = x.size(0)
        if x_0.dim() != 2 or x_0.size(1) != self.channels or x_0.size(0) < n:
            raise ValueError(f"GCN2Conv: x_0 must be [>= {n}, {self.channels}], got {tuple(x_0.shape)}")
        x_0 = x_0[:n]
        if n == 0:
            rel = None                            # nothing to propagate over and nothing to launch
        elif isinstance(edge_index, Relation):
            rel = edge_index                      # the caller built the structure, loops included
        else:
            rel = self_loop_relation_of(edge_index, n, both=torch.is_grad_enabled() and x.requires_grad)
        return Fh.GCN2ConvFn.apply(x, x_0, self.weight1, self.weight2, rel, self.alpha, self.beta, ACT[act])

    def __repr__(self) -> str:
        return f"GCN2Conv({self.channels}, alpha={self.alpha}, beta={self.beta})"


class GATConv(nn.Module):
    """PyG GATConv, heads=1, negative_slope=0.2, dropout=0, in its two uses:

    * ``add_self_loops=False``: the bipartite local->virtual relation (model/hscn.py:85-87, ``in_channels=(-1,-1)``)
      with two transforms ``lin_src`` / ``lin_dst`` (also for an int ``in_channels``) when called with a pair
      ``(x_src, x_dst)``; called with ONE Tensor (a homogeneous relation built with ``ll_conv`` / ``vv_conv`` = "GAT")
      ``lin_src`` transforms it for both roles, as PyG's forward does, and ``lin_dst`` is an unused parameter whose
      gradient stays ``None`` ("GATConv on one tensor");
    * ``add_self_loops=True`` (PyG's default, what ``MPNN`` constructs: model/mpnn.py:29-32) with an int
      ``in_channels``: a homogeneous graph, ONE transform (``lin_dst is lin_src``, as PyG builds it), input self
      loops removed and one loop per node appended.  ``state_dict`` carries the shared weight under both
      ``lin_src.weight`` and ``lin_dst.weight`` like PyG's; ``parameters()`` yields it once."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1,
                 negative_slope: float = 0.2, add_self_loops: bool = True, cached: bool = False,
                 bias: bool = True):
        super().__init__()
        if heads != 1:
            raise NotImplementedError("the hot path builds GATConv with heads=1")
        if add_self_loops and not isinstance(in_channels, int):
            raise NotImplementedError("GATConv(add_self_loops=True) is the homogeneous operator: int in_channels "
                                      "(a bipartite relation has no self loops to add)")
        self.add_self_loops = bool(add_self_loops)
        self.negative_slope = negative_slope
        self.out_channels = out_channels
        if self.add_self_loops:
            self.lin_src = Linear(in_channels, out_channels, bias=False, weight_initializer="glorot")
            self.lin_dst = self.lin_src
        else:
            if isinstance(in_channels, int):
                in_channels = (in_channels, in_channels)
            self.lin_src = Linear(in_channels[0], out_channels, bias=False, weight_initializer="glorot")
            self.lin_dst = Linear(in_channels[1], out_channels, bias=False, weight_initializer="glorot")
        self.att_src = nn.Parameter(_glorot(torch.empty(1, 1, out_channels)))
        self.att_dst = nn.Parameter(_glorot(torch.empty(1, 1, out_channels)))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index: Union[Tensor, Relation],
                act: str = "identity") -> Tensor:
        if self.add_self_loops:
            return self._forward_loops(x, edge_index, act)
        homogeneous = isinstance(x, Tensor)
        x_src, x_dst = (x, x) if homogeneous else x
        self.lin_src.materialize(x_src.size(-1), x_src)
        self.lin_dst.materialize(x_dst.size(-1), x_dst)
        rel = _relation(edge_index, x_src.size(0), x_dst.size(0), both=torch.is_grad_enabled())
        # ONE Tensor (HeteroConv's call when source and target type coincide): PyG transforms it once,
        # ``x_src = x_dst = lin_src(x)``; lin_dst keeps its state_dict entry, is not used and gets no gradient
        W_dst = self.lin_src.weight if homogeneous else self.lin_dst.weight
        return Fh.GATConvFn.apply(x_src, x_dst, self.lin_src.weight, W_dst, self.att_src,
                                  self.att_dst, self.bias, rel, self.negative_slope, ACT[act])

    def _forward_loops(self, x: Tensor, edge_index: Union[Tensor, Relation], act: str) -> Tensor:
        """``edge_index`` (or the Relation) is the RAW edge list: the loops are this layer's to add."""
        if not isinstance(x, Tensor):
            raise TypeError("GATConv(add_self_loops=True) takes one node feature tensor")
        self.lin_src.materialize(x.size(-1), x)
        n = x.size(0)
        both = torch.is_grad_enabled()
        rel = _relation(edge_index, n, n, both=both)
        if rel.num_src != n or rel.num_dst != n:
            raise ValueError(f"the relation is {rel.num_src} -> {rel.num_dst} nodes, x has {n} rows")
        loops = None
        if rel.max_in_degree > Fh.GAT_NARROW_MAX_DEGREE:    # one synchronising read per relation, then cached
            loops = self_loop_relation_of(rel.edge_index, n, both=both)
        return Fh.GATLoopFn.apply(x, self.lin_src.weight, self.att_src, self.att_dst, self.bias, rel, loops,
                                  self.negative_slope, ACT[act])


class ReLU(nn.Module):
    """``torch.nn.ReLU`` on the HIP path: the parameter-free middle module of GINE's ``Sequential``."""

    def forward(self, x: Tensor) -> Tensor:
        return Fh.ActFn.apply(x, ACT["relu"])


class GINEConv(nn.Module):
    """PyG GINEConv with ``edge_dim`` given: ``out = nn((1 + eps) x_i + sum_{k: dst_k = i} relu(x[src_k] +
    lin(edge_attr[k])))``, every edge as given (loops and repeated edges count).  ``lin = Linear(edge_dim, F)`` with
    bias, F being the input width of the first ``Linear`` found in ``nn`` as in PyG; ``edge_dim=-1`` is materialised
    on first use.  ``state_dict`` keys are PyG's: ``nn.*``, ``lin.weight``, ``lin.bias``, ``eps`` (a buffer).  The
    aggregate is one HIP launch (csrc/gine.hip), ``nn`` runs through its own modules.

    Not provided, refused by name: ``train_eps=True``, ``edge_dim=None`` (PyG's form without ``lin``, which needs
    edge features as wide as x) and a gradient for ``edge_attr``."""

    def __init__(self, nn_module: nn.Module, eps: float = 0.0, train_eps: bool = False, edge_dim: Optional[int] = None):
        super().__init__()
        if train_eps:
            raise NotImplementedError("GINEConv(train_eps=True): the gradient of eps is not computed; eps is a buffer")
        if edge_dim is None:
            raise NotImplementedError("GINEConv(edge_dim=None) adds raw edge features to x; pass edge_dim (or -1) so "
                                      "that they go through lin = Linear(edge_dim, in_channels)")
        self.nn = nn_module
        self.initial_eps = float(eps)
        self.register_buffer("eps", torch.tensor([float(eps)]))
        first = next((m for m in nn_module.modules() if isinstance(m, (Linear, nn.Linear))), None)
        if first is None:
            raise ValueError("GINEConv: no Linear found in nn to take the input width from")
        in_channels = first.in_channels if isinstance(first, Linear) else first.in_features
        if in_channels <= 0:
            raise ValueError("GINEConv: the first Linear of nn is lazily sized; lin needs its input width")
        self.in_channels = int(in_channels)
        self.lin = Linear(edge_dim, self.in_channels)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "eps" in state_dict:          # the launches take eps as a host value: no read-back per call
            self.initial_eps = float(state_dict[prefix + "eps"].reshape(-1)[0])

    def aggregate(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor) -> Tensor:
        if not isinstance(x, Tensor):
            raise TypeError("GINEConv takes one node feature tensor")
        if edge_attr is None:
            raise ValueError("GINEConv needs edge_attr [E, edge_dim]")
        if edge_attr.dim() != 2:
            raise ValueError(f"edge_attr must be [E, edge_dim], got {tuple(edge_attr.shape)}")
        self.lin.materialize(edge_attr.size(-1), x)
        n = x.size(0)
        # only a gradient w.r.t. x walks the source-keyed CSR
        rel = _relation(edge_index, n, n, both=torch.is_grad_enabled() and x.requires_grad)
        return Fh.GINEAggregateFn.apply(x, edge_attr, self.lin.weight, self.lin.bias, rel, self.initial_eps)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor) -> Tensor:
        return self.nn(self.aggregate(x, edge_index, edge_attr))


class GINE(GINEConv):
    """GraphGPS's GINE layer, constructible from ``(in, out)`` like the other registry entries: a ``GINEConv`` over
    ``Sequential(Linear(in, out), ReLU, Linear(out, out))``.  ``act`` is applied in the last Linear's epilogue."""

    uses_edge_attr = True

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int = -1, eps: float = 0.0):
        super().__init__(nn.Sequential(Linear(in_channels, out_channels), ReLU(), Linear(out_channels, out_channels)),
                         eps=eps, train_eps=False, edge_dim=edge_dim)
        self.out_channels = int(out_channels)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor,
                act: str = "identity") -> Tensor:
        z = self.aggregate(x, edge_index, edge_attr)
        return self.nn[2](self.nn[0](z, act="relu"), act=act)     # the middle ReLU in the first Linear's epilogue


def pna_avg_deg_log(deg) -> float:
    """PyG's ``avg_deg['log']`` from an in-degree histogram (``deg[d]`` = number of training nodes of in-degree d):
    the mean of ``log(d + 1)`` over the nodes, on the host in float64."""
    hist = [float(v) for v in (deg.tolist() if hasattr(deg, "tolist") else deg)]
    nodes = sum(hist)
    if not hist or any(v < 0 for v in hist) or nodes <= 0:
        raise ValueError("PNAConv: deg must be a histogram of in-degrees with at least one node")
    return sum(math.log(d + 1.0) * n for d, n in enumerate(hist)) / nodes


class PNAConv(nn.Module):
    """PyG PNAConv with ``towers=1, pre_layers=1, post_layers=1, divide_input=False`` (GraphGPS's configuration):

        m_k   = pre_nn(cat[x_i, x_j, edge_encoder(e_k)])          j = edge_index[0, k], i = edge_index[1, k]
        agg_i = cat over scalers s, aggregators x of  scaler_s(deg_i) * aggregator_x({m_k: dst_k = i})
        out_i = lin(post_nn(cat[x_i, agg_i]))

    every edge as given (loops and repeated edges count).  ``aggregators``: out of mean, min, max, sum, std
    (``sqrt(relu(mean(m^2) - mean(m)^2) + 1e-5)``); a node without in-edges gets 0, and ``sqrt(1e-5)`` for std.
    ``scalers``: identity, amplification ``log(d + 1) / avg_deg_log``, attenuation (its inverse), ``d = max(deg_i, 1)``;
    ``avg_deg_log`` is the training set's mean of ``log(deg + 1)``, given directly or through ``deg``, PyG's in-degree
    histogram, and required only beside a scaler other than identity.  Parameters and ``state_dict`` keys are PyG's:
    ``pre_nns.0.0`` = Linear(3F, F) (2F without ``edge_dim``), ``post_nns.0.0`` = Linear((S A + 1) F, out), ``lin`` =
    Linear(out, out), ``edge_encoder`` = Linear(edge_dim, F) (``-1`` is materialised on first use).

    The message is linear in its three parts, so the column blocks of the one ``pre_nns.0.0.weight`` are applied to
    the nodes and edges separately (``Linear``) and the reductions are one HIP launch that never writes the [E, F]
    messages (csrc/pna.hip).  min / max ties go to the first edge of the row in CSR order, and the gradient with
    them (torch's ``scatter_reduce`` splits it evenly).  ``edge_attr`` may carry a gradient.

    Not provided, refused by name: ``towers != 1``, ``pre_layers != 1``, ``post_layers != 1``, ``divide_input=True``,
    ``train_norm=True`` and the scalers ``linear`` and ``inverse_linear``."""

    def __init__(self, in_channels: int, out_channels: int, aggregators, scalers, deg=None,
                 edge_dim: Optional[int] = None, avg_deg_log: Optional[float] = None, towers: int = 1,
                 pre_layers: int = 1, post_layers: int = 1, divide_input: bool = False, train_norm: bool = False):
        super().__init__()
        if towers != 1:
            raise NotImplementedError(f"PNAConv(towers={towers}): one tower is provided (towers=1)")
        if pre_layers != 1:
            raise NotImplementedError(f"PNAConv(pre_layers={pre_layers}): the message is one Linear (pre_layers=1), "
                                      "which is what lets the operator reduce its three parts separately")
        if post_layers != 1:
            raise NotImplementedError(f"PNAConv(post_layers={post_layers}): one post Linear is provided (post_layers=1)")
        if divide_input:
            raise NotImplementedError("PNAConv(divide_input=True) splits the input between towers; one tower is provided")
        if train_norm:
            raise NotImplementedError("PNAConv(train_norm=True): a trainable avg_deg is not provided")
        aggregators, scalers = tuple(aggregators), tuple(scalers)
        for s in scalers:
            if s in ("linear", "inverse_linear"):
                raise NotImplementedError(f"PNAConv: the scaler {s!r} is not provided "
                                          f"(scalers are out of {Fh.PNA_SCALERS})")
        Fh.pna_codes(aggregators, scalers)
        in_channels, out_channels = int(in_channels), int(out_channels)
        if not 1 <= in_channels <= Fh.PNA_MAX_WIDTH:            # (the library's answer is asked at the first launch)
            raise ValueError(f"PNAConv: in_channels = {in_channels} outside the kernel's envelope ({Fh.PNA_ENVELOPE})")
        if avg_deg_log is None and deg is not None:
            avg_deg_log = pna_avg_deg_log(deg)
        if any(s != "identity" for s in scalers):
            if avg_deg_log is None:
                raise ValueError(f"PNAConv: scalers {scalers} need deg (the in-degree histogram of the training set) "
                                 "or avg_deg_log")
            if not 0.0 < float(avg_deg_log) < float("inf"):
                raise ValueError(f"PNAConv: avg_deg_log must be positive and finite, got {avg_deg_log!r}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggregators, self.scalers = aggregators, scalers
        self.avg_deg_log = None if avg_deg_log is None else float(avg_deg_log)
        self.edge_dim = edge_dim
        self.towers, self.divide_input = 1, False
        F = in_channels
        self.edge_encoder = Linear(edge_dim, F) if edge_dim is not None else None
        self.pre_nns = nn.ModuleList([nn.Sequential(Linear((3 if edge_dim is not None else 2) * F, F))])
        self.post_nns = nn.ModuleList([nn.Sequential(Linear((len(aggregators) * len(scalers) + 1) * F, out_channels))])
        self.lin = Linear(out_channels, out_channels)

    def aggregate(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Optional[Tensor] = None) -> Tensor:
        """[N, S A F]: the scaled aggregators of the messages."""
        if not isinstance(x, Tensor):
            raise TypeError("PNAConv takes one node feature tensor")
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"PNAConv: x must be [N, {self.in_channels}], got {tuple(x.shape)}")
        if self.edge_encoder is not None:
            if edge_attr is None:
                raise ValueError("PNAConv(edge_dim=...) needs edge_attr [E, edge_dim]")
            if edge_attr.dim() != 2:
                raise ValueError(f"edge_attr must be [E, edge_dim], got {tuple(edge_attr.shape)}")
            if not edge_attr.is_floating_point():
                raise TypeError(f"PNAConv: edge_attr must be float32, got {edge_attr.dtype}")
            self.edge_encoder.materialize(edge_attr.size(-1), x)
        elif edge_attr is not None:
            raise ValueError("PNAConv was built without edge_dim and cannot take edge_attr")
        n, F = x.size(0), self.in_channels
        grad = torch.is_grad_enabled()
        rel = _relation(edge_index, n, n, both=grad)
        if grad:
            rel.csr_t                       # (a relation built elsewhere without it: the source walk needs it)
        if edge_attr is not None and edge_attr.size(0) != rel.num_edges:
            raise ValueError(f"edge_attr is {tuple(edge_attr.shape)}; the relation has {rel.num_edges} edges")
        pre = self.pre_nns[0][0]
        a = Fh.linear_wide(x, pre.weight[:, :F], pre.bias)
        b = Fh.linear_wide(x, pre.weight[:, F:2 * F])
        t = None
        if self.edge_encoder is not None:
            e = Fh.linear_wide(edge_attr, self.edge_encoder.weight, self.edge_encoder.bias)
            t = Fh.linear_wide(e, pre.weight[:, 2 * F:])
        return Fh.PNAAggregateFn.apply(a, b, t, rel, self.aggregators, self.scalers, self.avg_deg_log)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Optional[Tensor] = None,
                act: str = "identity") -> Tensor:
        agg = self.aggregate(x, edge_index, edge_attr)
        post = self.post_nns[0][0]
        h = Fh.linear_wide(torch.cat([x, agg], -1), post.weight, post.bias)
        return Fh.linear_wide(h, self.lin.weight, self.lin.bias, act)


# what the registry's PNA layers are built with when no ``config.PNAConfig`` says otherwise
PNA_DEFAULT_AGGREGATORS = ("mean", "min", "max", "std")
PNA_DEFAULT_SCALERS = ("identity",)


class PNA(PNAConv):
    """GraphGPS's PNA layer without edge features, constructible from ``(in, out)`` like the other registry entries;
    ``aggregators`` / ``scalers`` / ``avg_deg_log`` are what a ``config.PNAConfig`` hands the model.  ``act`` is applied
    in the last Linear's epilogue."""

    def __init__(self, in_channels: int, out_channels: int, aggregators=PNA_DEFAULT_AGGREGATORS,
                 scalers=PNA_DEFAULT_SCALERS, avg_deg_log: Optional[float] = None, deg=None):
        super().__init__(in_channels, out_channels, aggregators, scalers, deg=deg, edge_dim=None,
                         avg_deg_log=avg_deg_log)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], act: str = "identity") -> Tensor:
        return super().forward(x, edge_index, None, act)


class PNAEdge(PNAConv):
    """The edge-aware PNA layer of the registry (as ``GINE`` is for ``GINEConv``): ``edge_dim=-1``, so ``edge_encoder``
    takes its input width from the first ``edge_attr``."""

    uses_edge_attr = True

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int = -1, aggregators=PNA_DEFAULT_AGGREGATORS,
                 scalers=PNA_DEFAULT_SCALERS, avg_deg_log: Optional[float] = None, deg=None):
        super().__init__(in_channels, out_channels, aggregators, scalers, deg=deg, edge_dim=edge_dim,
                         avg_deg_log=avg_deg_log)


class GatedGCNConv(nn.Module):
    """The bare convolution of GraphGPS's ``GatedGCNLayer`` (residual gated graph ConvNets), edge features in and out:

        e^_k = D x_i + E x_j + C e_k                  j = edge_index[0, k], i = edge_index[1, k]
        h_i  = A x_i + sum_k sigmoid(e^_k) * B x_j / (sum_k sigmoid(e^_k) + 1e-6)

    every edge as given (loops and repeated edges count).  Five ``Linear`` with bias under GraphGPS's names ``A, B, C,
    D, E`` (a ``state_dict`` moves across); ``C = Linear(edge_dim, out_channels)``, ``edge_dim=-1`` is materialised on
    first use.  The five transforms run through ``Linear``; the gates, the two sums and the new edge rows are one HIP
    launch (csrc/gatedgcn.hip).  ``forward`` returns ``(x_out, e_out)``, ``act`` applied to both; ``edge_attr`` may
    carry a gradient (the previous layer's edge output, a trainable edge encoder)."""

    uses_edge_attr = True
    updates_edge_attr = True

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int = -1):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.A = Linear(in_channels, out_channels)
        self.B = Linear(in_channels, out_channels)
        self.C = Linear(edge_dim, out_channels)
        self.D = Linear(in_channels, out_channels)
        self.E = Linear(in_channels, out_channels)

    def aggregate(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor) -> Tuple[Tensor, Tensor]:
        if not isinstance(x, Tensor):
            raise TypeError("GatedGCNConv takes one node feature tensor")
        if edge_attr is None:
            raise ValueError("GatedGCNConv needs edge_attr [E, edge_dim]")
        if edge_attr.dim() != 2:
            raise ValueError(f"edge_attr must be [E, edge_dim], got {tuple(edge_attr.shape)}")
        if not edge_attr.is_floating_point():
            raise TypeError(f"GatedGCNConv: edge_attr must be float32, got {edge_attr.dtype}")
        if not Fh.gatedgcn_supported(self.out_channels):
            raise ValueError(f"GatedGCNConv: width H={self.out_channels} outside the kernel's envelope "
                             f"(1 <= H <= {Fh.GATEDGCN_MAX_WIDTH})")
        self.C.materialize(edge_attr.size(-1), x)
        n = x.size(0)
        # a gradient w.r.t. Bx or Ex (their weights are parameters) walks the source-keyed CSR
        rel = _relation(edge_index, n, n, both=torch.is_grad_enabled())
        if edge_attr.size(0) != rel.num_edges:
            raise ValueError(f"edge_attr is {tuple(edge_attr.shape)}; the relation has {rel.num_edges} edges")
        return Fh.GatedGCNAggregateFn.apply(self.A(x), self.B(x), self.D(x), self.E(x), self.C(edge_attr), rel)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor,
                act: str = "identity") -> Tuple[Tensor, Tensor]:
        h, e = self.aggregate(x, edge_index, edge_attr)
        if act != "identity":
            h, e = Fh.ActFn.apply(h, ACT[act]), Fh.ActFn.apply(e, ACT[act])
        return h, e


class GatedGCNLayer(GatedGCNConv):
    """GraphGPS's ``GatedGCNLayer``: the convolution, then ``bn_node_x`` / ``bn_edge_e``, the activation and dropout on
    both the node and the edge output, then the residuals ``x_in + x`` and ``e_in + e`` (when ``residual`` is set and the
    widths agree).  Parameter names are GraphGPS's: ``A..E``, ``bn_node_x``, ``bn_edge_e``.  ``norm``: what
    ``nn.gps._norm`` accepts ("batch", "layer", None).  ``dropout_seed`` pins the masks (tests): the node mask draws
    with ``dropout_seed``, the edge mask with ``dropout_seed + EDGE_SEED_OFFSET``, far outside the consecutive seeds a
    model hands to its node masks."""

    EDGE_SEED_OFFSET = 1 << 20

    def __init__(self, channels: int, dropout: float = 0.0, residual: bool = True, norm: Optional[str] = "batch",
                 act: str = "relu", edge_dim: int = -1):
        super().__init__(channels, channels, edge_dim)
        from .gps import NORMS, _norm
        if norm not in NORMS:
            raise ValueError(f"norm must be 'layer', 'batch' or None, got {norm!r}")
        if act not in ACT:
            raise ValueError(f"act must be one of {sorted(ACT)}, got {act!r}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.channels, self.dropout, self.residual, self.act = int(channels), float(dropout), bool(residual), act
        self.dropout_seed: Optional[int] = None
        self.bn_node_x = _norm(norm, channels)
        self.bn_edge_e = _norm(norm, channels)

    def forward(self, x: Tensor, edge_index: Union[Tensor, Relation], edge_attr: Tensor) -> Tuple[Tensor, Tensor]:
        h, e = self.aggregate(x, edge_index, edge_attr)
        if self.bn_node_x is not None:
            h, e = self.bn_node_x(h), self.bn_edge_e(e)
        if self.act != "identity":
            h, e = Fh.ActFn.apply(h, ACT[self.act]), Fh.ActFn.apply(e, ACT[self.act])
        seed = self.dropout_seed
        h = Fh.dropout(h, p=self.dropout, training=self.training, seed=seed)
        e = Fh.dropout(e, p=self.dropout, training=self.training,
                       seed=None if seed is None else seed + self.EDGE_SEED_OFFSET)
        if self.residual:
            h = x + h
            if edge_attr.size(-1) == self.channels:
                e = edge_attr + e
        return h, e


class TransformerConv(nn.Module):
    """PyG TransformerConv with ``concat=True``, ``beta=False``, ``dropout=0``: multi-head scaled dot-product attention
    over the in-edges of every node, every edge as given (loops and repeated edges count),

        a_k   = softmax_k( lin_query(x_i) . (lin_key(x_j) + lin_edge(e_k)) / sqrt(C) )     per head, over dst_k = i
        out_i = sum_k a_k (lin_value(x_j) + lin_edge(e_k))  +  lin_skip(x_i)

    with ``heads`` heads of width ``C = out_channels`` (the output is ``[N, heads * out_channels]``).  Parameters and
    ``state_dict`` keys are PyG's: ``lin_key``, ``lin_query``, ``lin_value`` (bias), ``lin_edge`` (no bias, only with
    ``edge_dim``; ``-1`` is materialised on first use), ``lin_skip`` (only with ``root_weight``; ``bias`` is its
    bias).  Called with one Tensor or a pair ``(x_src, x_dst)``; ``in_channels`` may be an int, a pair, and ``-1`` is
    lazy.  The transforms run through ``Linear``, the softmax and both sums are one HIP launch
    (csrc/edge_attention.hip).  ``edge_attr`` may carry a gradient.

    Not provided, refused by name: ``concat=False``, ``beta=True`` and ``dropout > 0``."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1,
                 concat: bool = True, beta: bool = False, dropout: float = 0.0, edge_dim: Optional[int] = None,
                 bias: bool = True, root_weight: bool = True):
        super().__init__()
        if not concat:
            raise NotImplementedError("TransformerConv(concat=False): the mean over heads is not provided")
        if beta:
            raise NotImplementedError("TransformerConv(beta=True): the gated skip connection is not provided")
        if dropout:
            raise NotImplementedError("TransformerConv(dropout > 0): dropout on the attention weights is not provided")
        heads, out_channels = int(heads), int(out_channels)
        if heads < 1 or out_channels < 1:
            raise ValueError(f"TransformerConv: heads = {heads} and out_channels = {out_channels} must be positive")
        if heads * out_channels > Fh.EDGE_ATTN_MAX_WIDTH:       # (the library's answer is asked at the first launch)
            raise ValueError(f"TransformerConv: heads * out_channels = {heads * out_channels} outside the kernel's "
                             f"envelope ({Fh.EDGE_ATTN_ENVELOPE})")
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        self.in_channels, self.out_channels, self.heads = tuple(in_channels), out_channels, heads
        self.concat, self.beta, self.dropout = True, False, 0.0
        self.edge_dim, self.root_weight = edge_dim, bool(root_weight)
        width = heads * out_channels
        self.lin_key = Linear(in_channels[0], width)
        self.lin_query = Linear(in_channels[1], width)
        self.lin_value = Linear(in_channels[0], width)
        self.lin_edge = Linear(edge_dim, width, bias=False) if edge_dim is not None else None
        self.lin_skip = Linear(in_channels[1], width, bias=bias) if root_weight else None

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index: Union[Tensor, Relation],
                edge_attr: Optional[Tensor] = None, act: str = "identity") -> Tensor:
        x_src, x_dst = (x, x) if isinstance(x, Tensor) else x
        if self.lin_edge is not None:
            if edge_attr is None:
                raise ValueError("TransformerConv(edge_dim=...) needs edge_attr [E, edge_dim]")
            if edge_attr.dim() != 2:
                raise ValueError(f"edge_attr must be [E, edge_dim], got {tuple(edge_attr.shape)}")
            if not edge_attr.is_floating_point():
                raise TypeError(f"TransformerConv: edge_attr must be float32, got {edge_attr.dtype}")
        elif edge_attr is not None:
            raise ValueError("TransformerConv was built without edge_dim and cannot take edge_attr")
        # a gradient w.r.t. k or v (their weights are parameters) walks the source-keyed CSR
        rel = _relation(edge_index, x_src.size(0), x_dst.size(0), both=torch.is_grad_enabled())
        if edge_attr is not None and edge_attr.size(0) != rel.num_edges:
            raise ValueError(f"edge_attr is {tuple(edge_attr.shape)}; the relation has {rel.num_edges} edges")
        q, k, v = self.lin_query(x_dst), self.lin_key(x_src), self.lin_value(x_src)
        e = self.lin_edge(edge_attr) if self.lin_edge is not None else None
        out = Fh.EdgeAttentionFn.apply(q, k, v, e, rel, self.heads)
        if self.lin_skip is not None:
            out = out + self.lin_skip(x_dst)
        if act != "identity":
            out = Fh.ActFn.apply(out, ACT[act])
        return out


class EdgeTransformerConv(TransformerConv):
    """The edge-aware ``TransformerConv``, constructible from ``(in, out)`` like the other registry entries (as ``GINE``
    is for ``GINEConv``): ``edge_dim=-1``, so ``lin_edge`` takes its input width from the first ``edge_attr``."""

    uses_edge_attr = True

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int, heads: int = 1, **kwargs):
        kwargs.setdefault("edge_dim", -1)
        super().__init__(in_channels, out_channels, heads=heads, **kwargs)


class HeteroConv(nn.Module):
    """PyG HeteroConv(aggr='sum'): run each relation's conv in
    ``edge_index_dict`` order, sum the outputs that share a target type."""

    def __init__(self, convs: Dict[Tuple[str, str, str], nn.Module], aggr: str = "sum"):
        super().__init__()
        if aggr != "sum":
            raise NotImplementedError("HeteroConv on the hot path uses aggr='sum'")
        self.convs = nn.ModuleDict({"__".join(k): v for k, v in convs.items()})

    def forward(self, x_dict: Dict[str, Tensor], edge_index_dict: Dict[Tuple[str, str, str], Tensor]):
        outs: Dict[str, list] = {}
        for edge_type, edge_index in edge_index_dict.items():
            src, _, dst = edge_type
            key = "__".join(edge_type)
            if key not in self.convs:
                continue
            conv = self.convs[key]
            if src == dst:
                o = conv(x_dict[src], edge_index)
            else:
                o = conv((x_dict[src], x_dict[dst]), edge_index)
            outs.setdefault(dst, []).append(o)
        return {k: (v[0] if len(v) == 1 else torch.stack(v, 0).sum(0)) for k, v in outs.items()}
