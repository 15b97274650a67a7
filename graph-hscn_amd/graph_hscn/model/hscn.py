"""SCN (MinCUT spectral clustering net) and HSCN (heterogeneous local/virtual
message passing) with the reference's class names, constructor and ``forward``
signatures (/root/reference/graph_hscn/model/hscn.py:19-140), computing on
MI355X through the HIP C ABI (include/hscn.h).

Differences a caller can observe, all documented in DESIGN.md:
  * parameters are materialised eagerly (the reference's lazy ``-1`` dims
    materialise after the optimizer was built, train/train.py:155-159);
  * ``SCN.forward`` accepts an optional ``node_ptr`` to process a block-diagonal
    batch of graphs in one call (losses = mean over graphs); without it the call
    is the reference's single-graph step;
  * the dense ``[1,n,n]`` adjacency the reference returns and both callers drop
    (train/train_clustering.py:45,65) is built on the device only for
    single-graph calls; batched calls return ``None`` in that slot.
"""
from __future__ import annotations

import os

from typing import Callable, Dict, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from ..config.config import ACT_DICT, CONV_DICT, HSCNConfig
from ..nn import GATConv, GCNConv, GraphConv, HeteroConv, Linear, TransformerConv
from ..nn import functional as Fh
from ..nn.pool import (dmon_pool_sparse, global_mean_pool, mincut_pool_sparse, to_dense_adj, to_dense_adj_batched,
                       to_dense_adj_ragged)
from ..structure import Relation, relation_of
from .. import engine as _engine
from ._common import check_task_level

LL = ("local", "to", "local")
VV = ("virtual", "to", "virtual")
LV = ("local", "to", "virtual")
VL = ("virtual", "to", "local")      # extension (HSCN(vl_conv="GAT")): the lv edge list reversed
VL_NAME = "('virtual', 'to', 'local')"


def _act_name(act) -> Optional[str]:
    if isinstance(act, str):
        return act.lower()
    return getattr(act, "hscn_name", None)


class _MessagePassingStack(nn.Module):
    """Stand-in for PyG ``Sequential('x, edge_index, edge_weight', [...])``
    (hscn.py:28-45): GraphConv children are registered as ``module_{2i}`` so the
    ``state_dict`` keys equal the reference's."""

    def __init__(self, num_features: int, mp_units: list, act: str):
        super().__init__()
        self.act = act
        self.num = len(mp_units)
        dims = [num_features] + list(mp_units)
        for i in range(self.num):
            setattr(self, f"module_{2 * i}", GraphConv(dims[i], dims[i + 1]))

    def forward(self, x: Tensor, rel: Relation, edge_weight: Optional[Tensor]) -> Tensor:
        for i in range(self.num):
            x = getattr(self, f"module_{2 * i}")(x, rel, edge_weight, act=self.act)
        return x


class SCN(nn.Module):
    def __init__(self, mp_units: list, mp_act: str, num_features: int, num_clusters: int,
                 mlp_units: list = [], mlp_act: str = "identity", mincut_route: str = "sparse",
                 pool: str = "mincut"):
        """``mincut_route`` (extension): how ``dense_mincut_pool``'s contractions are evaluated.
        "sparse" -- on the edge list, A never densified (tr(S^T A S) = sum over edges of s_i . s_j; the fused
        graph-resident launch when the model has the reference's shape);
        "dense"  -- the reference's literal sequence ``to_dense_adj`` -> ``dense_mincut_pool`` (model/hscn.py:61-63)
        with the [B,n,n] adjacency materialised and A S, S^T (A S), S^T S, S^T X on the matrix cores (csrc/dense.hip,
        exact-fp32 MFMA): BASELINE.json configs[3], PascalVOC-SP with 64 clusters;
        "auto"   -- dense from 64 clusters on.  Same values either way (tests/test_gpu_models.py).

        ``pool`` (extension): the objective the assignment is fitted with.  "mincut" (default) is the reference's
        ``dense_mincut_pool`` pair, cut ratio + orthogonality.  "dmon" is DMoN (PyG ``dense_dmon_pool``): modularity
        with the degree null model, the same orthogonality term and a collapse regulariser on the cluster sizes
        (``nn.pool.dmon_pool_sparse``, csrc/dmon.hip).  It exists on the edge-list route and the layered operators
        only: ``forward`` then returns ``(S, spectral_loss, ortho_loss, cluster_loss, adj)`` and ``forward_graphs``
        ``(S, spectral, ortho, cluster[, total])`` with ``total`` the plain sum of the three."""
        super().__init__()
        if mincut_route not in ("sparse", "dense", "auto"):
            raise ValueError(f"mincut_route must be 'sparse', 'dense' or 'auto', not {mincut_route!r}")
        if pool not in ("mincut", "dmon"):
            raise ValueError(f"pool must be 'mincut' or 'dmon', not {pool!r}")
        self.mincut_route = mincut_route
        self.pool = pool
        self.num_clusters = int(num_clusters)
        if pool == "dmon" and self._dense():
            raise ValueError(f"pool='dmon': DMoN runs on the edge-list route only, there is no dense route for it "
                             f"(mincut_route={mincut_route!r} with {self.num_clusters} clusters selects the dense "
                             f"route; pass mincut_route='sparse')")
        if _act_name(mp_act) not in ACT_DICT or _act_name(mlp_act) not in ACT_DICT:
            raise KeyError(f"unknown activation {mp_act!r}/{mlp_act!r}")  # ACT_DICT[...] at hscn.py:34,53
        self.mp = _MessagePassingStack(num_features, mp_units, _act_name(mp_act))
        out_channels = mp_units[-1]
        self.mlp_act = _act_name(mlp_act)
        self.mlp = nn.Sequential()
        # hscn.py:50-53 keeps `out_channels` as the input width of every layer (the
        # notebook's `out_chan = units` got inverted); restated literally.
        for units in mlp_units:
            self.mlp.append(Linear(out_channels, units))
            self.mlp.append(nn.Identity())
        self.mlp.append(Linear(out_channels, num_clusters))
        # device flags of the ragged byte-adjacency route, OR-ed across the calls since the last check_adjacency():
        # bit 16 = a pair of nodes had more than 255 parallel edges (its entry saturated at 255, so that call's
        # losses are not the reference's).  Read at a point that synchronises anyway: the route never waits on the host.
        self.register_buffer("adj_flag", torch.zeros(1, dtype=torch.int32), persistent=False)

    def check_adjacency(self) -> None:
        """Raise if a byte adjacency of a dense-route call since the previous check saturated, and clear the flag
        (synchronises with the device).  Callers that run the byte route outside train_clustering call it where they
        read results back."""
        v = int(self.adj_flag.item())
        if v:
            self.adj_flag.zero_()
        if v & 16:
            raise OverflowError("dense MinCUT route: more than 255 parallel edges between two nodes saturated the byte "
                                "adjacency, so the losses differ from the reference's (set HSCN_DENSE_ADJ=f32)")

    def _dense(self) -> bool:
        return self.mincut_route == "dense" or (self.mincut_route == "auto" and self.num_clusters >= 64)

    def resident_ok(self, data) -> bool:
        """Can ``forward_graphs`` take the fused graph-resident path for this input?"""
        if self._dense():
            return False          # the dense route is the layered operators + the MFMA contractions
        if self.pool != "mincut":
            return False          # the one-launch stage-A kernels compute MinCUT's losses and nothing else
        layers = list(self.mlp)
        if self.mp.num != 1 or len(layers) != 1:
            return False
        conv = self.mp.module_0
        H, F = conv.lin_rel.weight.shape
        K = layers[0].weight.shape[0]
        meta = _engine.scn_meta(data, conv.lin_rel.weight.device)
        from .._hip import lib
        return bool(lib().hscn_scn_resident_supported(F, H, K, meta.max_n, meta.max_e))

    def forward_graphs(self, data, with_total: bool = False):
        """The body of the reference's clustering loop (train/train_clustering.py:37-47) for one
        ``Data`` graph or a block-diagonal ``Batch`` of RAW graphs: gcn_norm(add_self_loops=True),
        forward, MinCUT + orthogonality losses -- one fused launch when the model is the
        reference's shape (mp_units=[H], mlp_units=[]), else the layered operators.
        Returns ``(softmax [N,K], mc_loss, o_loss)`` (losses = mean over the graphs); with
        ``with_total`` also ``mc_loss + o_loss`` (train_clustering.py:48), which the fused launch
        produces itself -- no add launch, and its backward reaches the kernel as one scalar."""
        dev = self.mp.module_0.lin_rel.weight.device
        # the fused launch pair returns parameter gradients only: a differentiable input (something trainable feeds
        # the features) takes the layered operators, which return its gradient
        wants_x_grad = torch.is_grad_enabled() and data.x.requires_grad
        if wants_x_grad and data.x.dtype == torch.float16:
            raise RuntimeError("half-precision features that require grad: half storage runs on the fused stage-A "
                               "launch only, and that launch returns no gradient for its input features")
        if not wants_x_grad and self.resident_ok(data):
            conv, lin = self.mp.module_0, list(self.mlp)[0]
            meta = _engine.scn_meta(data, dev)
            x = data.x if data.x.is_cuda else data.x.to(dev)
            ei = data.edge_index if data.edge_index.is_cuda else data.edge_index.to(dev)
            if x.dtype != torch.float16:      # (half features stay half: include/hscn.h, HSCN_STORE_F16)
                x = x.float()
            S, mc, o, total = _engine.SCNResidentFn.apply(x, ei, meta, _engine.ACT[self.mp.act],
                                                          conv.lin_rel.weight, conv.lin_rel.bias, conv.lin_root.weight,
                                                          lin.weight, lin.bias)
            self.last_engine = "resident"
            return (S, mc, o, total) if with_total else (S, mc, o)
        from ..nn.pool import gcn_norm, gcn_norm_static
        self.last_engine = "layered"
        if data.x.dtype == torch.float16:
            raise RuntimeError("half-precision feature storage runs on the fused stage-A launch only (mp_units=[H], "
                               "mlp_units=[], graphs that fit one CU's LDS)")
        raw_ei = data.edge_index if data.edge_index.is_cuda else data.edge_index.to(dev)
        N = int(data.num_nodes)
        batched = "ptr" in data and data.ptr is not None
        if not self._dense():
            ei, ew = gcn_norm(raw_ei, None, N, add_self_loops=True)
            node_ptr = data.ptr.to(dev).to(torch.int32) if batched else None
            if self.pool == "dmon":
                S, sp, o, cl, _ = self.forward(data.x.to(dev).float(), ei, ew, node_ptr=node_ptr)
                return (S, sp, o, cl, sp + o + cl) if with_total else (S, sp, o, cl)
            S, mc, o, _ = self.forward(data.x.to(dev).float(), ei, ew, node_ptr=node_ptr)
            return (S, mc, o, mc + o) if with_total else (S, mc, o)
        # dense route: gcn_norm(add_self_loops=True) in its static-shape form and A + I straight from the raw edges --
        # every launch has a shape known on the host, so the whole step (forward, losses, backward) can be captured
        # and replayed as one hipGraph; graphs of any sizes share a batch
        ei, ew = gcn_norm_static(raw_ei, None, N)
        cached = getattr(data, "_dense_seg", None)
        if cached is None or cached[0].device != dev:
            if batched:
                cached = (data.ptr.to(dev).to(torch.int32).contiguous(), data.batch.to(dev).to(torch.int32).contiguous(),
                          int(data.max_nodes))
            else:
                cached = (torch.tensor([0, N], dtype=torch.int32, device=dev),
                          torch.zeros(N, dtype=torch.int32, device=dev), N)
            try:
                data._dense_seg = cached
            except AttributeError:
                pass
        node_ptr, gid, nmax = cached
        S, mc, o, _ = self.forward(data.x.to(dev).float(), ei, ew, node_ptr=node_ptr, nodes_per_graph=nmax,
                                   node_graph=gid, raw_edge_index=raw_ei)
        return (S, mc, o, mc + o) if with_total else (S, mc, o)

    def forward(self, x: Tensor, edge_index: Tensor, edge_weight: Optional[Tensor],
                node_ptr: Optional[Tensor] = None, nodes_per_graph: Optional[int] = None,
                node_graph: Optional[Tensor] = None, raw_edge_index: Optional[Tensor] = None):
        """Batched calls of the dense route (extensions; the reference's own call is one graph at a time):
        ``nodes_per_graph`` = the LARGEST node count of the batch's graphs (the common one when they are equal),
        ``node_graph`` int32 [N] = graph of every node -- needed when the graphs differ in size: the adjacency is then
        [B, nmax, nmax] with zeros beyond each graph, node-indexed tensors stay flat, and every graph's loss terms
        equal the single-graph call's.  ``raw_edge_index``: the edge list BEFORE gcn_norm added self loops, when
        ``edge_index`` came from ``gcn_norm_static`` (whose zero-weight placeholders must not be counted)."""
        n = x.size(0)
        rel = relation_of(edge_index, n, n)
        x = self.mp(x.float(), rel, edge_weight)
        s = x
        layers = list(self.mlp)
        for i, m in enumerate(layers):
            if isinstance(m, Linear):
                last = i == len(layers) - 1
                s = m(s, act="identity" if last else self.mlp_act)
        if self._dense():
            # model/hscn.py:61-63 literally: adj = to_dense_adj(edge_index); dense_mincut_pool(x, adj, s)
            if node_ptr is None:
                Bg, ng = 1, n
            else:
                Bg = int(node_ptr.numel()) - 1
                ng = int(nodes_per_graph) if nodes_per_graph else 0
                if ng <= 0:
                    raise ValueError("the dense MinCUT route on a batch needs nodes_per_graph (the largest graph's node "
                                     "count: it sizes the [B,n,n] adjacency)")
            if node_ptr is not None and (Bg * ng != n or raw_edge_index is not None):
                if node_graph is None:
                    raise ValueError("graphs of different sizes on the dense MinCUT route need node_graph (int32 [N])")
                # ragged batch: A + I of every graph in its own [nmax, nmax] block, node-indexed tensors flat
                # (the adjacency as bytes: nobody outside this call sees it -- batched calls return None in its slot --
                # and the products that stream it move a quarter of the bytes; HSCN_DENSE_ADJ=f32 keeps floats)
                as_bytes = os.environ.get("HSCN_DENSE_ADJ", "u8") != "f32"
                want_sym = as_bytes
                flag = self.adj_flag if as_bytes else None
                if raw_edge_index is not None:
                    adj = to_dense_adj_ragged(raw_edge_index, node_ptr, node_graph, Bg, ng, raw=True, as_bytes=as_bytes,
                                              flag=flag, symmetry=want_sym)
                else:
                    adj = to_dense_adj_ragged(edge_index, node_ptr, node_graph, Bg, ng, as_bytes=as_bytes, flag=flag,
                                              symmetry=want_sym)
                # byte route: one pass flags the graphs whose adjacency is not symmetric; the others (undirected graphs:
                # the norm) take the backward's A^T S from the forward's A S
                asym = None
                if want_sym:
                    adj, asym = adj
                S, mc_loss, o_loss, _, _ = Fh.MinCutDenseRaggedFn.apply(s, x, adj, node_ptr, node_graph, asym)
                self.last_route = "dense-ragged"
                return S, mc_loss, o_loss, None
            adj = to_dense_adj_batched(edge_index, Bg, ng)
            S, mc_loss, o_loss, _, _ = Fh.MinCutDenseFn.apply(s.view(Bg, ng, -1), x.view(Bg, ng, -1), adj)
            self.last_route = "dense"
            return S.view(n, -1), mc_loss, o_loss, (adj if node_ptr is None else None)
        self.last_route = "sparse"
        if self.pool == "dmon":
            S, _, _, sp_loss, o_loss, cl_loss = dmon_pool_sparse(x, rel, s, node_ptr)
            adj = to_dense_adj(edge_index, n) if node_ptr is None else None
            return S, sp_loss, o_loss, cl_loss, adj
        S, _, _, mc_loss, o_loss = mincut_pool_sparse(x, rel, s, node_ptr)
        adj = to_dense_adj(edge_index, n) if node_ptr is None else None
        return S, mc_loss, o_loss, adj


def build_conv_relation(conv_type: str, hidden_channels: int, in_channels=None, heads: int = 1) -> nn.Module:
    """hscn.py:117-125.  ``in_channels`` (extension) materialises the lazy ``-1``.  ``heads`` (extension): the attention
    heads of "TransformerConv", ``heads`` heads of width ``hidden_channels // heads``."""
    if conv_type.lower() == "transformerconv_edge":
        raise ValueError("conv_type 'TransformerConv_edge' needs edge features, and the hetero graph carries no edge "
                         "features yet (HeteroData has no edge_attr; the MPNN baseline and GPS take "
                         "'transformerconv_edge', the relations take 'TransformerConv')")
    if heads != 1 and conv_type.lower() != "transformerconv":
        raise ValueError(f"heads={heads} needs conv_type 'TransformerConv', not {conv_type!r}")
    if conv_type.lower() == "transformerconv":
        if heads < 1 or hidden_channels % heads:
            raise ValueError(f"hidden_channels {hidden_channels} must be divisible by heads {heads}")
        dim = -1 if in_channels is None else (in_channels, in_channels)
        return TransformerConv(dim, hidden_channels // heads, heads=heads)     # (no add_self_loops / cached: not its)
    if conv_type.lower() == "gatedgcn":
        raise ValueError("conv_type 'GatedGCN' needs edge features, and the hetero graph carries no edge features yet "
                         "(HeteroData has no edge_attr; the MPNN baseline and GPS take 'gatedgcn')")
    if conv_type.lower() in ("pna", "pna_edge"):
        raise ValueError(f"conv_type {conv_type!r}: HSCN's relations do not take PNAConv yet (the MPNN baseline and GPS "
                         "take 'pna' and 'pna_edge')")
    if conv_type.lower() == "gine":
        raise ValueError("conv_type 'GINE' needs edge features, and the hetero graph carries no edge features yet "
                         "(HeteroData has no edge_attr; the MPNN baseline takes conv_type 'gine')")
    if conv_type == "GAT":
        dim = (-1, -1) if in_channels is None else (in_channels, in_channels)
    else:
        dim = -1 if in_channels is None else in_channels
    return CONV_DICT[conv_type.lower()](dim, hidden_channels, add_self_loops=False, cached=False)


class HSCN(nn.Module):
    def __init__(self, lv_conv: str, ll_conv: str, vv_conv: str, activation: Callable, num_features: int,
                 hidden_channels: int, num_classes: int, num_layers: int, vl_conv: Optional[str] = None,
                 task_level: str = "graph", heads: int = 1) -> None:
        """``heads`` (extension): the attention heads of the relations built as "TransformerConv" (lv, ll, vv; ``heads``
        heads of width ``hidden_channels // heads``); such a model runs on the layered operators.

        ``task_level`` (extension; the default "graph" is the reference's model): "node" skips the mean pool and
        applies the head ``lin_2(act(lin_1(.)))`` to every local node, returning ``[N, C]`` (``nn.head.NodeHead``: the
        one-launch head where ``hscn_node_head_supported`` says so, else the two ``Linear`` modules).  The convolution
        stack runs on the layered operators; the graph-resident launches, which end in the pooled head, refuse such a
        model.  "link": ``num_classes`` is the embedding width D; ``embed`` is exactly the node-level model's forward
        (the same ``NodeHead``, the same state_dict keys) and ``forward`` scores the batch's candidate pairs
        ``batch["local"].edge_label_index`` by the dot product of their embeddings (``nn.head.pair_dot``), giving [P].

        ``vl_conv`` (extension; the default ``None`` is the reference's model, bit for bit): "GAT" gives every
        layer a fourth convolution on the relation ("virtual", "to", "local") -- the lv edge list reversed, derived in
        ``forward`` when the batch does not carry it -- so that the clusters act as long-range shortcuts and the
        virtual branch reaches the prediction.  Every local node has exactly one such in-edge, so the attention weight
        is exactly 1 and the relation computes ``lin_src(x_virtual)[cluster(i)] + bias``: its ``lin_dst``,
        ``att_src`` and ``att_dst`` receive exactly zero gradients (zero, not ``None``).  The last layer's lv and vv
        convolutions still do not reach ``pred`` (``grad`` stays ``None``).  Per type the relation outputs are summed
        ``local = ll + vl`` and ``virtual = vv + lv``, then the reference's hard ReLU."""
        super().__init__()
        if vl_conv is not None and vl_conv != "GAT":
            raise ValueError(f"vl_conv must be None or 'GAT', not {vl_conv!r} (a bipartite GCNConv does not exist)")
        check_task_level(task_level)
        if heads != 1 and not any(c.lower() == "transformerconv" for c in (lv_conv, ll_conv, vv_conv)):
            raise ValueError(f"heads={heads} needs a relation built as 'TransformerConv'")
        self.vl_conv = vl_conv
        self.task_level = task_level
        self.heads = int(heads)

        def rel_heads(conv_type):
            return self.heads if conv_type.lower() == "transformerconv" else 1
        self.activation = activation
        self.convs = nn.ModuleList()
        for layer in range(num_layers):
            fin = num_features if layer == 0 else hidden_channels
            rels = {
                LV: build_conv_relation(lv_conv, hidden_channels, fin, heads=rel_heads(lv_conv)),
                LL: build_conv_relation(ll_conv, hidden_channels, fin, heads=rel_heads(ll_conv)),
                VV: build_conv_relation(vv_conv, hidden_channels, fin, heads=rel_heads(vv_conv)),
            }
            if vl_conv is not None:
                rels[VL] = build_conv_relation(vl_conv, hidden_channels, fin)
            self.convs.append(HeteroConv(rels, aggr="sum"))
        self.lin_1 = Linear(hidden_channels, hidden_channels)
        self.lin_2 = Linear(hidden_channels, num_classes)
        # execution engine: "auto" picks the graph-resident fused kernels when the batch
        # qualifies (engine.py), else the per-operator (layered) path; both are HIP.
        self.engine = "auto"
        self.compute_virtual = True   # the reference evaluates the virtual branch although pred ignores it
        self.keep_virtual = False     # expose the final virtual features as self.last_virtual
        # resident engine: run the virtual branch as its own launch beside loss + backward (engine.py)
        self.overlap_virtual = os.environ.get("HSCN_OVERLAP_VIRTUAL", "1") != "0"
        self.last_virtual: Optional[Tensor] = None
        self.last_engine: Optional[str] = None
        self.node_head = None
        if task_level != "graph" and _act_name(activation) in ACT_DICT:
            from ..nn.head import NodeHead
            # (a plain object: the parameters stay lin_1 / lin_2 and the state_dict the graph-level model's)
            self.node_head = NodeHead(self.lin_1, self.lin_2, _act_name(activation))

    NODE_LEVEL_REASON = ("a node-level head (task_level='node'): the one-launch and graph-resident kernels end in the "
                         "mean pool and the per-graph head, a per-node prediction runs on the layered operators")

    LINK_LEVEL_REASON = ("a link-level head (task_level='link'): the one-launch and graph-resident kernels end in the "
                         "mean pool and the per-graph head, a score per candidate pair runs on the layered operators and "
                         "the pair decoder")

    def _refuse_node_level(self, what: str) -> None:
        """The resident launches pool: they must refuse a node-level or link-level model, never pool silently."""
        if self.task_level == "node":
            raise RuntimeError(f"{what} does not take this model: {self.NODE_LEVEL_REASON}")
        if self.task_level == "link":
            raise RuntimeError(f"{what} does not take this model: {self.LINK_LEVEL_REASON}")

    def _refuse_vl(self, what: str) -> None:
        """The hscn_resident_* launches know three relations: they must refuse a model with a fourth, never drop it."""
        extra = [k for conv in self.convs for k in conv.convs if k not in ("__".join(LV), "__".join(LL), "__".join(VV))]
        if self.vl_conv is not None or extra:
            raise RuntimeError(f"{what} does not take a model with the relation {VL_NAME} (vl_conv={self.vl_conv!r}): "
                               "its launches evaluate ll, vv and lv only; this model's one-launch step is "
                               "step.VLResidentTrainStep, its forward-only launch hscn_vl_forward")

    def _resident_plan(self, x_dict, edge_index_dict, batch):
        if self.engine == "layered":
            return None
        if self.task_level != "graph":
            if self.engine == "resident":
                self._refuse_node_level("engine='resident'")
            return None
        if self.vl_conv is not None:
            if self.engine == "resident":
                self._refuse_vl("the graph-resident engine (hscn_resident_*)")
            return None
        # the launch pair returns parameter gradients only (HSCNResidentFn.backward): with a differentiable feature
        # input -- a trainable node encoder in front of the model -- "auto" takes the layered operators, which return
        # that gradient, and "resident" refuses rather than cut the graph silently
        if torch.is_grad_enabled() and any(isinstance(v, Tensor) and v.requires_grad for v in x_dict.values()):
            which = sorted(k for k, v in x_dict.items() if isinstance(v, Tensor) and v.requires_grad)
            if any(x_dict[k].dtype == torch.float16 for k in which):
                raise RuntimeError(f"half-precision node features that require grad ({which}): half storage runs on "
                                   "the graph-resident engine only, and that engine returns no gradient for its "
                                   "feature inputs")
            if self.engine == "resident":
                raise RuntimeError(f"engine='resident' requested but the node features {which} require grad: the "
                                   "graph-resident launches return no gradient for their feature inputs "
                                   "(engine='auto' or 'layered' runs the layered operators, which do)")
            return None
        name = _act_name(self.activation)
        ok = (name in ACT_DICT and set(edge_index_dict) == {LL, VV, LV} and "local" in x_dict
              and "virtual" in x_dict and x_dict["local"].is_cuda)
        ok = ok and self._resident_params() is not None
        meta = _engine.meta_from_batch(batch, x_dict["local"].device) if ok else None
        H, C = self.lin_1.out_channels, self.lin_2.out_channels
        if meta is None or not _engine.supported(x_dict["local"].size(1), H, len(self.convs), C, meta,
                                                 x_dict["local"].dtype):
            if self.engine == "resident":
                raise RuntimeError("engine='resident' requested but the batch/model does not qualify "
                                   "(needs a graph_hscn HeteroBatch, GAT/GCN/GCN relations, H in {16,32,64}, "
                                   "F <= H and graphs that fit one CU's LDS)")
            return None
        return meta, name

    def _resident_params(self):
        """The parameter order the resident launches take, or None when the relations are not the
        GAT / GCN / GCN combination; looked up once (the eager path is host-bound), rebuilt when the module
        tree changes (load_state_dict keeps the Parameter objects, assigning new modules does not)."""
        key = tuple(id(m) for conv in self.convs for m in conv.convs.values()) + (id(self.lin_1.weight), id(self.lin_2.weight))
        cached = getattr(self, "_resident_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        self._refuse_vl("the graph-resident engine (hscn_resident_*)")
        params = []
        for conv in self.convs:
            c = conv.convs
            ll, vv, lv = (c["__".join(k)] for k in (LL, VV, LV))
            if not (isinstance(ll, GCNConv) and isinstance(vv, GCNConv) and isinstance(lv, GATConv)):
                params = None
                break
            params += [ll.lin.weight, ll.bias, vv.lin.weight, vv.bias, lv.lin_src.weight, lv.lin_dst.weight,
                       lv.att_src, lv.att_dst, lv.bias]
        if params is not None:
            params += [self.lin_1.weight, self.lin_1.bias, self.lin_2.weight, self.lin_2.bias]
        object.__setattr__(self, "_resident_cache", (key, params))
        return params

    def _forward_resident(self, x_dict, edge_index_dict, meta, act_name) -> Tensor:
        params = self._resident_params()
        slope = self.convs[0].convs["__".join(LV)].negative_slope
        cfg = (_engine.ACT[act_name], slope, self.compute_virtual, self.keep_virtual, self.overlap_virtual)
        out = _engine.HSCNResidentFn.apply(x_dict["local"], x_dict["virtual"], edge_index_dict[LL],
                                           edge_index_dict[VV], edge_index_dict[LV], meta, cfg, *params)
        out, xv, score = out
        if xv is not None:
            self.last_virtual = xv
        if score is not None:
            # loss.criterion recognises a prediction that comes with its score and lets the loss tail ride on
            # the backward launch (no launch of its own)
            out._hscn_score = (score, out._version)
        return out

    # ---- the model with the virtual -> local relation (vl_conv="GAT") ----
    def vl_params(self):
        """Parameters in the order the hscn_vl_* launches take them: per layer {W_ll, b_ll, W_vv, b_vv, lv: W_src,
        W_dst, att_src, att_dst, b, vl: the same five}, then W1, b1, W2, b2."""
        out = []
        for conv in self.convs:
            c = conv.convs
            ll, vv, lv, vl = (c["__".join(k)] for k in (LL, VV, LV, VL))
            out += [ll.lin.weight, ll.bias, vv.lin.weight, vv.bias]
            for gat in (lv, vl):
                out += [gat.lin_src.weight, gat.lin_dst.weight, gat.att_src, gat.att_dst, gat.bias]
        return out + [self.lin_1.weight, self.lin_1.bias, self.lin_2.weight, self.lin_2.bias]

    def vl_grad_order(self):
        """The parameters in the order of the launch's flat gradient buffer: ``vl_params()`` with the last layer's
        dead part (``vl_dead_params()``) moved behind the head, so that the live gradients tile the buffer's front."""
        dead = {id(p) for p in self.vl_dead_params()}
        allp = self.vl_params()
        return [p for p in allp if id(p) not in dead] + [p for p in allp if id(p) in dead]

    def vl_dead_params(self):
        """The parameters the prediction does not depend on (autograd leaves their ``grad`` at None): the last layer's
        vv and lv convolutions."""
        vv, lv = (self.convs[-1].convs["__".join(k)] for k in (VV, LV))
        return [vv.lin.weight, vv.bias, lv.lin_src.weight, lv.lin_dst.weight, lv.att_src, lv.att_dst, lv.bias]

    def resident_reason(self, batch=None, x_dict=None) -> Optional[str]:
        """Why this model (and ``batch``, if given) cannot take the one-launch hscn_vl_* kernels, or None when it
        can.  ``hscn_vl_supported`` is the single source of truth for the sizes."""
        from .._hip import lib
        if self.task_level == "node":
            return self.NODE_LEVEL_REASON
        if self.task_level == "link":
            return self.LINK_LEVEL_REASON
        if self.vl_conv is None:
            return f"the model has no {VL_NAME} relation (the hscn_resident_* launches serve the reference's model)"
        if _act_name(self.activation) not in ACT_DICT:
            return f"head activation {self.activation!r} (relu, elu, identity and tanh are supported)"
        slopes = set()
        for conv in self.convs:
            c = conv.convs
            if sorted(c) != sorted("__".join(k) for k in (LL, VV, LV, VL)):
                return "relations other than ll, vv, lv and vl"
            ll, vv, lv, vl = (c["__".join(k)] for k in (LL, VV, LV, VL))
            if not (isinstance(ll, GCNConv) and isinstance(vv, GCNConv) and isinstance(lv, GATConv)
                    and isinstance(vl, GATConv)) or ll.add_self_loops or vv.add_self_loops or lv.add_self_loops \
                    or vl.add_self_loops or any(m.bias is None for m in (ll, vv, lv, vl)):
                return "convolutions other than GCN (ll, vv) / GAT (lv, vl) without self loops, with bias"
            slopes.add(float(lv.negative_slope))
        if len(slopes) != 1:
            return "the lv convolutions differ in negative_slope"
        H, C, L = self.lin_1.out_channels, self.lin_2.out_channels, len(self.convs)
        F = int(self.convs[0].convs["__".join(LL)].lin.weight.shape[1])
        env = "H in {16, 32}, F <= H, C <= min(H, 16), 1 <= L <= 8"
        if batch is None:
            return None if lib().hscn_vl_supported(F, H, L, C, 0, 0, 0, 0) else \
                f"widths F={F}, H={H}, C={C}, L={L} outside the kernel's envelope ({env})"
        x_dict = x_dict if x_dict is not None else batch.x_dict
        xl, xv = x_dict.get("local"), x_dict.get("virtual")
        if xl is None or xv is None or not xl.is_cuda or xl.dtype != torch.float32 or xv.dtype != torch.float32 \
                or xl.dim() != 2 or xl.size(1) != F or xv.size(1) != F:
            return "node features must be float32 [N, F] / [V, F] tensors on the HIP device"
        meta = _engine.meta_from_batch(batch, xl.device)
        if meta is None:
            return "the batch carries no per-graph segment tables (graph_hscn.data.HeteroBatch builds them)"
        y = batch["local"].y if "y" in batch["local"] else None
        if y is not None and (y.dim() != 2 or y.size(1) != C):
            return "class-index (multiclass) targets: the fused loss row takes [B, C] multilabel / regression targets"
        if not lib().hscn_vl_supported(F, H, L, C, meta.max_n, meta.max_v, meta.max_ell, meta.max_evv):
            return (f"widths F={F}, H={H}, C={C}, L={L} or the largest graph ({meta.max_n} nodes, {meta.max_v} clusters, "
                    f"{meta.max_ell} / {meta.max_evv} edges) outside the kernel's envelope ({env}, 160 KB of LDS)")
        return None

    def supported(self, batch=None) -> bool:
        """Whether the one-launch hscn_vl_* kernels take this model (and ``batch``)."""
        return self.resident_reason(batch) is None

    def _forward_vl_resident(self, x_dict, edge_index_dict, batch) -> Tensor:
        from .._hip import call, ptr, stream
        xl, xv = x_dict["local"].contiguous(), x_dict["virtual"].contiguous()
        dev = xl.device
        meta = _engine.meta_from_batch(batch, dev)
        ei = [edge_index_dict[k].contiguous() for k in (LL, VV, LV)]
        params = [p.detach().contiguous() for p in self.vl_params()]
        L = len(self.convs)
        H, C = self.lin_1.out_channels, self.lin_2.out_channels
        pred = torch.empty(meta.num_graphs, C, dtype=torch.float32, device=dev)
        xv_out = torch.empty(max(xv.size(0), 1), H, dtype=torch.float32, device=dev) if self.keep_virtual else None
        slope = float(self.convs[0].convs["__".join(LV)].negative_slope)
        call("hscn_vl_forward", ptr(xl), ptr(xv), ptr(ei[0]), ei[0].size(1), ptr(ei[1]), ei[1].size(1), ptr(ei[2]),
             ei[2].size(1), ptr(meta.lptr), ptr(meta.vptr), ptr(meta.eptr_ll), ptr(meta.eptr_vv), ptr(meta.eptr_lv),
             xl.size(0), xv.size(0), meta.num_graphs, xl.size(1), H, L, C, _engine.ACT[_act_name(self.activation)], slope,
             _engine._ptr_table(params[:14 * L]), *[ptr(p) for p in params[14 * L:]], meta.max_n, meta.max_v,
             meta.max_ell, meta.max_evv, None, 0, 0.0, ptr(pred), None, None, None, ptr(xv_out), ptr(meta.flag), stream())
        if xv_out is not None:
            self.last_virtual = xv_out
        return pred

    def _forward_vl(self, x_dict, edge_index_dict, batch) -> Tensor:
        if self.engine not in ("layered", "auto", "resident"):
            raise ValueError(f"engine must be 'layered', 'auto' or 'resident', got {self.engine!r}")
        if self.engine == "resident":
            self._refuse_node_level("engine='resident'")
        if not self.compute_virtual:
            raise ValueError(f"compute_virtual=False is meaningless with the relation {VL_NAME}: the local update "
                             "reads the virtual features of every layer")
        if VL not in edge_index_dict:        # the data layer does not change: vl is lv reversed, appended last
            edge_index_dict = dict(edge_index_dict)
            edge_index_dict[VL] = edge_index_dict[LV].flip(0)
        if self.engine != "layered" and self.task_level == "graph":
            if torch.is_grad_enabled():
                if self.engine == "resident":
                    self._refuse_vl("engine='resident' with gradients on (the hscn_resident_* autograd launches)")
            else:
                reason = self.resident_reason(batch, x_dict)
                if reason is None:
                    self.last_engine = "resident"
                    return self._forward_vl_resident(x_dict, edge_index_dict, batch)
                if self.engine == "resident":
                    raise RuntimeError(f"engine='resident' requested but the model / batch does not qualify: {reason}")
        return self._forward_layered(x_dict, edge_index_dict, batch)

    def forward(self, x_dict: Dict[str, Tensor], edge_index_dict: Dict[Tuple[str, str, str], Tensor],
                batch) -> Tensor:
        out = self._forward(x_dict, edge_index_dict, batch)
        if self.task_level == "link":                  # one score per candidate pair of the batch
            from ..nn.head import PairStructure, pair_dot
            local = batch["local"]
            return pair_dot(out, local.edge_label_index, PairStructure.of(local, out.size(0)))
        return out

    def embed(self, x_dict: Dict[str, Tensor], edge_index_dict: Dict[Tuple[str, str, str], Tensor],
              batch) -> Tensor:
        """The [N, D] node embeddings a link-level model scores pairs with: the node-level model's forward."""
        if self.task_level != "link":
            raise RuntimeError("embed() belongs to a link-level model (task_level='link')")
        return self._forward(x_dict, edge_index_dict, batch)

    def _forward(self, x_dict, edge_index_dict, batch) -> Tensor:
        if self.vl_conv is not None:
            return self._forward_vl(x_dict, edge_index_dict, batch)
        plan = self._resident_plan(x_dict, edge_index_dict, batch)
        if plan is not None:
            self.last_engine = "resident"
            return self._forward_resident(x_dict, edge_index_dict, *plan)
        return self._forward_layered(x_dict, edge_index_dict, batch)

    def _forward_layered(self, x_dict, edge_index_dict, batch) -> Tensor:
        self.last_engine = "layered"
        if x_dict["local"].dtype == torch.float16:
            raise RuntimeError("half-precision feature storage runs on the graph-resident engine only (H in {16, 32}, "
                               "a graph_hscn HeteroBatch, graphs that fit one CU's LDS)")
        relu = ACT_DICT["relu"]
        for conv in self.convs:
            x_dict = conv(x_dict, edge_index_dict)
            x_dict = {key: relu(x) for key, x in x_dict.items()}           # hscn.py:110 (hard-coded ReLU)
        name = _act_name(self.activation)
        if self.task_level != "graph":                                     # the head on every local node: no pool
            x = x_dict["local"]
            if self.node_head is not None:
                return self.node_head(x)
            return self.lin_2(self.activation(self.lin_1(x)))
        local = batch["local"]
        size = getattr(batch, "num_graphs", None) or None
        x = global_mean_pool(x_dict["local"], local.batch, size)           # hscn.py:111
        if name is not None:
            x = self.lin_1(x, act=name)                                    # hscn.py:112 fused epilogue
        else:
            x = self.activation(self.lin_1(x))
        return self.lin_2(x)                                               # hscn.py:113


def build_hscn(model_cfg: HSCNConfig, num_features: int, num_classes: int) -> HSCN:
    return HSCN(
        model_cfg.lv_conv_type,
        model_cfg.ll_conv_type,
        model_cfg.vv_conv_type,
        ACT_DICT[model_cfg.activation.lower()],
        num_features,
        model_cfg.hidden_channels,
        num_classes,
        model_cfg.num_layers,
        getattr(model_cfg, "vl_conv_type", None),
        getattr(model_cfg, "task_level", "graph"),
        getattr(model_cfg, "heads", 1),
    )
