"""The GPS model (extension; the reference has no global attention): ``Linear(F -> D)`` node encoder, ``num_layers``
``nn.gps.GPSLayer`` s -- a local convolution beside per-graph multi-head self-attention -- and a head per task level:

  * "graph": ``global_mean_pool -> Linear(D, D) -> activation -> Linear(D, C)`` (HSCN's head shape);
  * "node":  the same two Linears per node, through ``nn.head.NodeHead`` where its kernels apply;
  * "link":  ``embed()`` is the [N, C] output of the two Linears and ``forward`` scores ``batch.edge_label_index`` by
    ``nn.head.pair_dot``: ``model/_common.py LinkLevel``, which ``MPNN`` shares.

``local_conv=None`` is the plain Transformer (with a positional encoding in front: LRGB's "Transformer + LapPE").
The model takes a homogeneous ``Batch`` and offers the surface ``train.batching`` and ``train.train`` use for one.  It
runs on the layered operators only: there is no one-launch or captured form of global attention.

``node_encoder="atom"`` / ``edge_encoder="bond"`` put OGB's categorical encoders (``encoder/categorical.py``) in place of
the Linear node / edge encoder; ``batch.x`` / ``batch.edge_attr`` are then int64 categories."""
from __future__ import annotations

from typing import Callable, Optional

import torch.nn as nn
from torch import Tensor

from ..config.config import ACT_DICT, GPSConfig, check_exphormer
from ..encoder.categorical import EDGE_ENCODERS
from ._common import LayeredModel, _Table  # noqa: F401  (_Table stays importable from here)
from ..nn import functional as Fh
from ..nn.conv import Linear
from ..nn.gps import GPSLayer
from ..structure import ExphormerStructure

EXPHORMER_RESIDENT_REASON = ("Exphormer's sparse attention (model/gps.py GPS, global_model='exphormer'): typed edge "
                            "attention over the union of local, expander and virtual-node edges has no one-launch, "
                            "resident or captured form; the model runs on the layered operators")
RESIDENT_REASON = ("global attention (model/gps.py GPS): per-graph multi-head self-attention has no one-launch, "
                   "resident or captured form; the model runs on the layered operators")


class GPS(LayeredModel):
    def __init__(self, num_features: int, hidden_channels: int, num_classes: int, num_layers: int, num_heads: int = 4,
                 local_conv: Optional[str] = "gine", activation: Optional[Callable] = None, dropout: float = 0.0,
                 norm: Optional[str] = "layer", task_level: str = "graph", node_encoder: Optional[str] = None,
                 edge_encoder: Optional[str] = None, attn_bias: Optional[str] = None, spd_max_dist: int = 20,
                 global_model: str = "attention", expander_degree: int = 6, num_virtual_nodes: int = 1,
                 add_local_edges: bool = True, expander_seed: int = 0, pos_enc=None, pe_undirected: bool = True,
                 pna=None) -> None:
        """``pna`` (a ``config.PNAConfig`` or None): the aggregators, scalers and ``avg_deg_log`` of every layer's local
        branch with ``local_conv`` "pna" / "pna_edge" (None: the layer's defaults).

        ``pos_enc`` (a ``config.LapPEConfig`` or ``config.RWSEConfig`` with ``dim_emb = hidden_channels``): the model
        owns a trainable positional encoder ``pe_encoder`` (``model/_common.py PosEnc``); the node encoder is built at
        width ``D - dim_pe`` and the layers see ``[h | pe]``.  The statistics are the batch's own or computed once per
        batch on the device (``pe_undirected``: the edge list holds both directions).  It combines with ``attn_bias``
        and ``global_model`` freely.

        ``global_model="exphormer"``: every layer's global branch is ``nn.attention.ExphormerAttention`` over the
        union of the batch's own edges (``add_local_edges``), a random ``expander_degree``-regular expander drawn under
        ``expander_seed`` and ``num_virtual_nodes`` virtual nodes per graph.  The model then owns
        ``virt_node_emb.weight`` [nv, D] (the virtual rows every graph starts from) and ``edge_type_emb.weight``
        [2 + 2 nv, D] (the features of the edges that have none of their own), builds the batch's
        ``structure.ExphormerStructure`` once (kept on the batch, ``graph_ids = arange(B)``), carries the virtual rows
        from layer to layer and hands heads and pooling the node rows only.  The local edges' own features reach the
        attention where the model encodes edge features to width D: the ``edge_encoder`` ("bond") or "gatedgcn"'s
        edge state as they are, and for the other edge-aware convolutions ("gine", "transformerconv_edge") a
        ``Linear(-1, D)`` of the attention's own, ``exph_edge_encoder``; without an edge-aware ``local_conv`` the local
        edges share type 0 of the table.  The four further arguments are read by "exphormer" only.

        ``attn_bias="spd"``: Graphormer's spatial encoding -- every layer's attention owns a table
        ``layers.i.attn.spd_bias.weight`` [spd_max_dist + 1, num_heads] added to its logits by shortest-path bucket; the
        model builds the batch's buckets once per forward (``nn.functional.shortest_path_buckets``, cached on the
        batch per ``spd_max_dist``) and hands them to all layers.

        ``node_encoder="atom"`` / ``edge_encoder="bond"``: an ``AtomEncoder(D)`` / ``BondEncoder(D)`` over int64
        categories in place of the Linear node / edge encoder (for "gine" the bond encoder supplies the ``edge_attr``
        the layer's own edge Linear reads).  The defaults build the model as it always was."""
        super().__init__()
        self._check_args(node_encoder, edge_encoder, task_level, num_layers)
        if attn_bias not in (None, "spd"):
            raise ValueError(f"attn_bias must be 'spd' or None, not {attn_bias!r}")
        if attn_bias is not None and not Fh.SPD_MIN_DIST <= int(spd_max_dist) <= Fh.SPD_MAX_DIST:
            raise ValueError(f"spd_max_dist must be in [{Fh.SPD_MIN_DIST}, {Fh.SPD_MAX_DIST}], got {spd_max_dist}")
        if global_model not in ("attention", "exphormer"):
            raise ValueError(f"global_model must be 'attention' or 'exphormer', not {global_model!r}")
        self.global_model = global_model
        if global_model == "exphormer":
            if attn_bias is not None:
                raise ValueError(f"global_model='exphormer' and attn_bias={attn_bias!r} do not go together: the "
                                 "shortest-path bias belongs to the dense attention (attn_bias must be None)")
            check_exphormer(expander_degree, num_virtual_nodes)
        self.expander_degree, self.num_virtual_nodes = int(expander_degree), int(num_virtual_nodes)
        self.add_local_edges, self.expander_seed = bool(add_local_edges), int(expander_seed)
        self.attn_bias = attn_bias
        self.spd_max_dist = int(spd_max_dist)
        # (pinned masks: layer i draws with dropout_seed + 4 i .. + 4 i + 3)
        self._record(task_level, num_layers, activation, dropout, node_encoder, edge_encoder)
        act = self.activation.hscn_name
        D = int(hidden_channels)
        self._build_node_encoder(num_features, D, pos_enc, pe_undirected)
        spd_buckets = self.spd_max_dist + 1 if attn_bias == "spd" else None
        if global_model == "exphormer":
            self.layers = nn.ModuleList(GPSLayer(D, local_conv, num_heads, dropout, norm, act, global_model="exphormer",
                                                 num_virtual_nodes=self.num_virtual_nodes, pna=pna)
                                        for _ in range(num_layers))
        else:
            self.layers = nn.ModuleList(GPSLayer(D, local_conv, num_heads, dropout, norm, act, spd_buckets=spd_buckets,
                                                 pna=pna) for _ in range(num_layers))
        if edge_encoder is not None:
            if not self.layers[0].uses_edge_attr:
                raise ValueError(f"edge_encoder={edge_encoder!r} needs an edge-aware local_conv ('gine', 'gatedgcn', "
                                 f"'transformerconv_edge' or 'pna_edge'), "
                                 f"not {local_conv!r}")
            self.edge_encoder = EDGE_ENCODERS[edge_encoder](D)
        elif self.layers[0].updates_edge_attr:      # "gatedgcn": edge features are a state of width D
            self.edge_encoder = Linear(-1, D)
        self._build_head(D, num_classes)
        if global_model == "exphormer":             # after every parameter of before
            self.virt_node_emb = _Table(self.num_virtual_nodes, D)
            self.edge_type_emb = _Table(2 + 2 * self.num_virtual_nodes, D)
            if self.layers[0].uses_edge_attr and not hasattr(self, "edge_encoder") and self.add_local_edges:
                self.exph_edge_encoder = Linear(-1, D)
        self._build_pos_encoder(D)                  # after every parameter of before

    # ---- what LayeredModel asks of the model ---------------------------------------------------------------------
    def _own_reason(self) -> str:
        return EXPHORMER_RESIDENT_REASON if self.global_model == "exphormer" else RESIDENT_REASON

    def _check_launch_flags(self, dev) -> None:
        """An attention launch that met a graph larger than its batch's ``max_nodes``."""
        Fh.check_attention(dev)
        if self.global_model == "exphormer":        # and the expander launches' (a graph beyond max_nodes)
            Fh.check_expander(dev)
        if self.attn_bias == "spd":                 # and the bucket launches' (an edge outside its graph, max_nodes)
            Fh.check_spd(dev)

    def _edge_attr_reader(self) -> str:
        return f"the model has edge-aware convolutions (local_conv {self.layers[0].local_conv!r})"

    # ---- forward -----------------------------------------------------------------------------------------------
    def _spd(self, batch):
        """The batch's ``SPDBuckets`` at ``spd_max_dist``, built once: kept on the batch object, in a dict that
        ``train.batching.to_device`` hands on by reference, keyed by ``(max_dist, device)`` -- a batch reused across
        epochs (resident on the device, or moved there every step from the same host batch) is not computed again."""
        if self.attn_bias != "spd":
            return None
        cache = getattr(batch, "__dict__", {}).setdefault("_spd_cache", {})
        key = (self.spd_max_dist, str(batch.ptr32.device))
        if key not in cache:
            cache[key] = Fh.shortest_path_buckets(batch, self.spd_max_dist)
        return cache[key]

    def _nodes(self, batch) -> Tensor:
        """[N, D] after the last GPS layer."""
        sparse = self.global_model == "exphormer"
        glob = {"spd": self._spd(batch)}            # the global branch's keywords, once per forward for all layers
        edge_attr = self._edge_attr(batch) if self.layers[0].uses_edge_attr else None
        x = self.encode_nodes(batch)
        if self.layers[0].updates_edge_attr or self.encoder_kinds[1] is not None:
            edge_attr = self.edge_encoder(edge_attr)
        if sparse:                                  # the virtual rows travel beside the node rows and stay behind
            # the local edges' own features reach the attention at width D (see __init__); otherwise they share type 0
            wide = hasattr(self, "edge_encoder") and self.layers[0].uses_edge_attr
            own = self.add_local_edges and (wide or hasattr(self, "exph_edge_encoder"))
            struct = ExphormerStructure.of(batch, self.expander_degree, self.num_virtual_nodes, self.add_local_edges,
                                           self.expander_seed, edge_features=own)
            e_static = self.exph_edge_encoder(edge_attr) if own and not wide else None
            virt = self.virt_node_emb.weight.repeat(struct.num_graphs, 1)  # graph-major: row g nv + t = weight[t]
            e_type = self.edge_type_emb.weight
        for i, layer in enumerate(self.layers):
            layer.dropout_seed = None if self.dropout_seed is None else self.dropout_seed + 4 * i
            if sparse:                              # (a layer that updates the edge features hands on the new ones)
                glob = {"exph": (struct, virt, (edge_attr if wide else e_static) if own else None, e_type)}
            out = layer(x, batch.edge_index, batch, edge_attr, **glob)
            out = out if isinstance(out, tuple) else (out,)                 # h; (h, e); (h, virt); (h, e, virt)
            x = out[0]
            if layer.updates_edge_attr:             # the layer's new edge features feed the next layer
                edge_attr = out[1]
            if sparse:
                virt = out[-1]
        return x


def build_gps(model_cfg: GPSConfig, num_features: int, num_classes: int) -> GPS:
    return GPS(num_features, model_cfg.hidden_channels, num_classes, model_cfg.num_layers, model_cfg.num_heads,
               model_cfg.local_conv_type, ACT_DICT[model_cfg.activation.lower()], model_cfg.dropout, model_cfg.norm,
               model_cfg.task_level, getattr(model_cfg, "node_encoder", None), getattr(model_cfg, "edge_encoder", None),
               getattr(model_cfg, "attn_bias", None), getattr(model_cfg, "spd_max_dist", 20),
               getattr(model_cfg, "global_model", "attention"), getattr(model_cfg, "expander_degree", 6),
               getattr(model_cfg, "num_virtual_nodes", 1), getattr(model_cfg, "add_local_edges", True),
               getattr(model_cfg, "expander_seed", 0), getattr(model_cfg, "pos_enc", None),
               getattr(model_cfg, "pe_undirected", True), getattr(model_cfg, "pna", None))
