"""The MPNN baseline with the reference's signature (model/mpnn.py:13-78; BASELINE config 1,
configs/GCN/peptides_func_GCN.yaml): ``num_layers`` convolutions ``F -> H -> ... -> C``, each hidden
one followed by ReLU, the configured activation and dropout, then a per-graph mean of the last
convolution's node outputs.  Everything numerical runs in the HIP library: GCNConv (transform +
normalised CSR gather-reduce with the ReLU in its epilogue), the activation, the counter-based
dropout and the segment mean.

Normalisation layers (model/mpnn.py:34-44,53-56) are built and applied exactly as the reference does, quirk
included: BOTH module lists -- ``bns`` (BatchNorm1d) and ``lns`` (LayerNorm) -- are created under ``use_layer_norm``
(mpnn.py:35 tests the wrong flag), so ``use_batch_norm=True`` alone reads a ``self.bns`` that does not exist and the
forward raises AttributeError, as the reference's does.  The layers compute through csrc/norm.hip.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn
from torch import Tensor

from .. import _hip
from ..config.config import ACT_DICT, CONV_DICT, MPNNConfig, pna_kwargs
from ..encoder.categorical import EDGE_ENCODERS, NODE_ENCODERS, resident_reason as encoder_reason
from ..nn.conv import GCNConv, Linear, PNAConv, TransformerConv
from ..nn import functional as Fh
from ..nn.norm import BatchNorm1d, LayerNorm
from ..nn.pool import global_mean_pool
from ._common import POSENC_RESIDENT_REASON, LinkLevel, PosEnc, check_encoders, check_task_level, float_edge_attr


class MPNN(LinkLevel, PosEnc, nn.Module):
    def __init__(self, conv: type, activation: Callable, num_features: int, hidden_channels: int,
                 num_classes: int, num_layers: int, dropout: float = 0.0, use_batch_norm: bool = False,
                 use_layer_norm: bool = False, task_level: str = "graph", node_encoder: Optional[str] = None,
                 edge_encoder: Optional[str] = None, heads: int = 1, pos_enc=None, pe_undirected: bool = True,
                 pna=None) -> None:
        """``pna`` (extension; a ``config.PNAConfig`` or None): with a PNA ``conv`` (``PNA`` / ``PNAEdge``) every layer is
        built with its aggregators, scalers and ``avg_deg_log`` (None: the layer's defaults); such a model is
        layered-only.

        ``pos_enc`` (extension; a ``config.LapPEConfig`` or ``config.RWSEConfig`` with ``dim_emb = hidden_channels``):
        the model owns a trainable positional encoder ``pe_encoder`` (``model/_common.py PosEnc``).  The node features
        are embedded to ``hidden_channels - dim_pe`` columns -- by the ``AtomEncoder`` of ``node_encoder="atom"``, else
        by a new ``linear_x = Linear(F, H - dim_pe)`` -- the encoder's ``dim_pe`` columns are appended and the first
        convolution is ``H -> H``, the shape ``node_encoder="atom"`` already gives it.  Such a model is layered-only.

        ``heads`` (extension): with a multi-head ``conv`` (``TransformerConv`` / ``EdgeTransformerConv``) the hidden
        layers are ``conv(in, hidden_channels // heads, heads=heads)`` and the last one ``conv(hidden, num_classes,
        heads=1)``; such a model is layered-only.

        ``task_level`` (extension; the default "graph" is the reference's model): "node" returns the last
        convolution's ``[N, C]`` without the per-graph mean.  "link": ``num_classes`` is the embedding width D,
        ``embed`` is that node-level output and ``forward`` scores the batch's candidate pairs
        ``batch.edge_label_index`` by the dot product of their embeddings (``nn.head.pair_dot``), giving [P]; both are
        ``model/_common.py LinkLevel``'s.

        ``node_encoder="atom"`` (extension): ``batch.x`` holds int64 categories, an ``AtomEncoder(hidden_channels)``
        embeds them and the first convolution is ``H -> H``.  ``edge_encoder="bond"``: a ``BondEncoder(hidden_channels)``
        embeds the int64 ``batch.edge_attr`` for the edge-aware convolutions.  Either makes the model layered-only."""
        super().__init__()
        check_task_level(task_level)
        check_encoders(node_encoder, edge_encoder)
        if edge_encoder is not None and not getattr(conv, "uses_edge_attr", False):
            raise ValueError(f"edge_encoder={edge_encoder!r} needs an edge-aware convolution (conv_type 'gine', "
                             f"'gatedgcn', 'transformerconv_edge' or 'pna_edge'), not {getattr(conv, '__name__', conv)}")
        multi_head = isinstance(conv, type) and issubclass(conv, TransformerConv)
        is_pna = isinstance(conv, type) and issubclass(conv, PNAConv)
        if pna is not None and not is_pna:
            raise ValueError(f"pna=PNAConfig(...) needs a PNA convolution (conv_type 'pna' or 'pna_edge'), not "
                             f"{getattr(conv, '__name__', conv)}")
        if not isinstance(heads, int) or heads < 1:
            raise ValueError(f"heads must be a positive int, not {heads!r}")
        if heads != 1 and not multi_head:
            raise ValueError(f"heads={heads} needs a multi-head convolution (conv_type 'transformerconv' or "
                             f"'transformerconv_edge'), not {getattr(conv, '__name__', conv)}")
        if hidden_channels % heads:
            raise ValueError(f"hidden_channels {hidden_channels} must be divisible by heads {heads}")
        self.heads = heads
        self.task_level = task_level
        self.num_layers = num_layers
        self.encoder_kinds = (node_encoder, edge_encoder)
        if node_encoder is not None or edge_encoder is not None or multi_head or is_pna:
            # train.batching.refuse_layered_only: the resident and device-dataset entry points refuse this model by name
            self.layered_only = True
        x_width = self._init_pos_enc(pos_enc, pe_undirected, hidden_channels)     # H - dim_pe with a positional encoder
        in_features = num_features
        if node_encoder is not None:
            self.node_encoder = NODE_ENCODERS[node_encoder](x_width)
        if node_encoder is not None or pos_enc is not None:
            num_features = hidden_channels
        if edge_encoder is not None:
            self.edge_encoder = EDGE_ENCODERS[edge_encoder](hidden_channels)
        self.conv_layers = nn.ModuleList()                                  # mpnn.py:27-32
        if multi_head:
            self.conv_layers.append(conv(num_features, hidden_channels // heads, heads=heads))
            for _ in range(num_layers - 2):
                self.conv_layers.append(conv(hidden_channels, hidden_channels // heads, heads=heads))
            self.conv_layers.append(conv(hidden_channels, num_classes, heads=1))
        else:
            kw = pna_kwargs(pna)
            self.conv_layers.append(conv(num_features, hidden_channels, **kw))
            for _ in range(num_layers - 2):
                self.conv_layers.append(conv(hidden_channels, hidden_channels, **kw))
            self.conv_layers.append(conv(hidden_channels, num_classes, **kw))
        self.use_batch_norm = use_batch_norm
        if use_layer_norm:                                                  # mpnn.py:35-38 (sic: not use_batch_norm)
            self.bns = nn.ModuleList(BatchNorm1d(hidden_channels) for _ in range(num_layers - 1))
        self.use_layer_norm = use_layer_norm
        if use_layer_norm:                                                  # mpnn.py:41-44
            self.lns = nn.ModuleList(LayerNorm(hidden_channels) for _ in range(num_layers - 1))
        self.activation = activation
        self.dropout = dropout
        self.dropout_seed: Optional[int] = None     # tests pin the mask; None = torch.initial_seed() + call counter
        # execution engine of the forward: "layered" (per-operator kernels, the default), "auto" / "resident" (with
        # gradients off, a qualifying Batch runs as ONE launch, include/hscn.h: hscn_mpnn_forward; "resident" raises
        # with the reason when the model or batch does not qualify).  Training with gradients on stays layered; the
        # fused training step is step.MPNNResidentTrainStep (autograd passes through the layered kernels).
        self.engine = "layered"
        self.last_engine: Optional[str] = None
        if pos_enc is not None:                     # after every parameter of before
            if node_encoder is None:
                self.linear_x = Linear(in_features, x_width)
            self._build_pos_encoder(hidden_channels)

    def resident_reason(self, batch=None, need_grad: bool = False) -> Optional[str]:
        """Why this model (and ``batch``, if given) cannot take the one-launch MPNN kernels, or None when it can."""
        if self.pos_enc is not None:
            return POSENC_RESIDENT_REASON + ("; " + encoder_reason(*self.encoder_kinds) if any(self.encoder_kinds) else "")
        for c in self.conv_layers:
            if isinstance(c, TransformerConv):
                return (f"convolution {type(c).__name__} (multi-head attention over the in-edges has no one-launch, "
                        "resident or captured form; the model runs on the layered operators)")
            if isinstance(c, PNAConv):
                return ("convolution PNAConv (the multi-aggregator reduction over the in-edges has no one-launch, "
                        "resident or captured form; the model runs on the layered operators)")
        if any(self.encoder_kinds):
            return encoder_reason(*self.encoder_kinds)
        if self.task_level == "node":
            return ("a node-level head (task_level='node'): the one-launch kernels end in the per-graph mean, a "
                    "per-node prediction runs on the layered operators")
        if self.task_level == "link":
            return ("a link-level head (task_level='link'): the one-launch kernels end in the per-graph mean, a "
                    "score per candidate pair runs on the layered operators and the pair decoder")
        name = getattr(self.activation, "hscn_name", None)
        if name not in ("relu", "elu", "identity", "tanh"):
            return f"activation {name!r} (relu, elu, identity and tanh are supported)"
        if self.use_batch_norm or self.use_layer_norm:
            return "normalisation layers (use_batch_norm / use_layer_norm) are not part of the fused kernel"
        for c in self.conv_layers:
            if not isinstance(c, GCNConv) or not c.add_self_loops or c.bias is None:
                return f"convolution {type(c).__name__} (only GCNConv(add_self_loops=True) with bias)"
            if isinstance(c.lin.weight, nn.parameter.UninitializedParameter):
                return "lazily sized convolution weights are not materialised yet"
        L = self.num_layers
        if L < 2 or len(self.conv_layers) != L:
            return "fewer than two convolutions"
        F, H, C = self.resident_dims()
        if batch is None:
            ok = _hip.lib().hscn_mpnn_supported(F, H, L, C, 0, 0)
            return None if ok else f"widths F={F}, H={H}, C={C}, L={L} outside the kernel's envelope (H in {{16, 32}}, F <= H, C <= min(H, 16), L <= 8)"
        for attr in ("ptr32", "eptr32", "max_nodes", "max_edges"):
            if not hasattr(batch, attr):
                return f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)"
        y = getattr(batch, "y", None)
        if y is not None and (y.dim() != 2 or y.size(1) != C):
            return "class-index (multiclass) targets: the fused loss row takes [B, C] multilabel / regression targets"
        x = batch.x
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != F:
            return "node features must be a float32 [N, F] tensor on the HIP device"
        if not _hip.lib().hscn_mpnn_supported(F, H, L, C, int(batch.max_nodes), int(batch.max_edges)):
            return (f"widths F={F}, H={H}, C={C}, L={L} or the largest graph ({batch.max_nodes} nodes, "
                    f"{batch.max_edges} edges) outside the kernel's envelope (160 KB of LDS)")
        return None

    def supported(self, batch=None) -> bool:
        """Whether the one-launch MPNN kernels take this model (and ``batch``)."""
        return self.resident_reason(batch) is None

    def resident_dims(self):
        first, last = self.conv_layers[0], self.conv_layers[-1]
        return int(first.lin.weight.shape[1]), int(first.lin.weight.shape[0]), int(last.lin.weight.shape[0])

    def resident_params(self):
        """Parameters in the order the fused kernels take them: {W_l, b_l} per convolution (= ``parameters()``)."""
        out = []
        for c in self.conv_layers:
            out += [c.lin.weight, c.bias]
        return out

    def _forward_resident(self, batch) -> Tensor:
        from .. import engine as _engine
        x = batch.x.contiguous()
        ei = batch.edge_index.contiguous()
        dev = x.device
        F, H, C = self.resident_dims()
        B = int(batch.num_graphs)
        params = [p.detach().contiguous() for p in self.resident_params()]
        table = _engine._ptr_table(params)
        ptr32 = batch.ptr32 if batch.ptr32.device == dev else batch.ptr32.to(dev)
        eptr32 = batch.eptr32 if batch.eptr32.device == dev else batch.eptr32.to(dev)
        pred = torch.empty(B, C, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _hip.call("hscn_mpnn_forward", _hip.ptr(x), _hip.ptr(ei), ei.size(1), _hip.ptr(ptr32), _hip.ptr(eptr32),
                  x.size(0), B, F, H, self.num_layers, C, _hip.ACT[self.activation.hscn_name], table,
                  int(batch.max_nodes), int(batch.max_edges), None, 0, 0.0, _hip.ptr(pred), None, None, None,
                  _hip.ptr(flag), _hip.stream())
        self._resident_flag = flag     # nonzero: an edge outside its graph / a graph beyond the batch's maxima
        return pred

    def check_flags(self) -> None:
        """Synchronising, for a model with a categorical encoder only: raises ``IndexError`` if a launch since the last
        check met a category outside its column's range (``nn.functional.check_categorical``).  ``train.train_epoch``
        / ``eval_epoch`` call it once per epoch; a model without an encoder has no flag word and nothing is read."""
        if any(self.encoder_kinds):
            Fh.check_categorical(next(self.parameters()).device)
        self._check_pe_flags()                      # the positional encoder's statistics launches, where there is one

    def _embed_x(self, batch) -> Tensor:
        if self.encoder_kinds[0] is not None:
            return self.node_encoder(batch.x)
        return self.linear_x(batch.x) if self.pos_enc is not None else batch.x

    def _edge_attr(self, batch) -> Tensor:
        """``batch.edge_attr`` for the layers with ``uses_edge_attr``: float32 [E, De] on the model's device (with an
        edge encoder: the int64 categories, embedded)."""
        ea = getattr(batch, "edge_attr", None)
        if ea is None:
            kind = "gatedgcn" if any(getattr(c, "updates_edge_attr", False) for c in self.conv_layers) else \
                ("transformerconv_edge" if isinstance(self.conv_layers[0], TransformerConv) else
                 ("pna_edge" if isinstance(self.conv_layers[0], PNAConv) else "gine"))
            raise ValueError(f"the model has edge-aware convolutions (conv_type {kind!r}) and the batch carries no "
                             "edge_attr (Data(edge_attr=[E, De]); make_dataset(..., edge_features=True))")
        if self.encoder_kinds[1] is not None:
            return self.edge_encoder(ea)
        return float_edge_attr(ea, next(self.parameters()).device)

    def _forward(self, batch) -> Tensor:
        if self.engine not in ("layered", "auto", "resident"):
            raise ValueError(f"engine must be 'layered', 'auto' or 'resident', got {self.engine!r}")
        if self.engine == "resident" and (self.task_level != "graph" or getattr(self, "layered_only", False)):
            raise RuntimeError(f"engine='resident' does not take this model: {self.resident_reason()}")
        if self.engine != "layered" and not torch.is_grad_enabled():
            reason = self.resident_reason(batch)
            if reason is None and self.training and self.dropout > 0:
                reason = "dropout in training mode (the forward-only launch is for evaluation)"
            if reason is None:
                self.last_engine = "resident"
                return self._forward_resident(batch)
            if self.engine == "resident":
                raise RuntimeError(f"engine='resident' requested but the model / batch does not qualify: {reason}")
        self.last_engine = "layered"
        edge_index, batch_vec = batch.edge_index, batch.batch               # mpnn.py:50
        x = self.encode_nodes(batch)                                        # batch.x, or [embedded x | pe]
        edge_attr = self._edge_attr(batch) if any(getattr(c, "uses_edge_attr", False) for c in self.conv_layers) else None

        def conv(i, x, **kw):                                               # edge-aware layers also take edge_attr
            nonlocal edge_attr
            c = self.conv_layers[i]
            if getattr(c, "updates_edge_attr", False):                      # "gatedgcn": (x, e); e feeds the next layer
                x, edge_attr = c(x, edge_index, edge_attr, **kw)            # (the last layer's e is dropped)
                return x
            return c(x, edge_index, edge_attr, **kw) if getattr(c, "uses_edge_attr", False) else c(x, edge_index, **kw)
        act_name = getattr(self.activation, "hscn_name", None)
        for i in range(self.num_layers - 1):
            x = conv(i, x, act="relu")                                      # F.relu(conv(x)) in the epilogue
            if self.use_batch_norm:
                x = self.bns[i](x)                                          # mpnn.py:53-54
            if self.use_layer_norm:
                x = self.lns[i](x)                                          # mpnn.py:55-56
            normed = self.use_batch_norm or self.use_layer_norm             # (a normalised x is no longer >= 0)
            if normed or act_name not in ("relu", "identity", "elu"):       # relu / elu are the identity on x >= 0
                x = self.activation(x)
            seed = None if self.dropout_seed is None else self.dropout_seed + i
            x = Fh.dropout(x, p=self.dropout, training=self.training, seed=seed)
        x = conv(self.num_layers - 1, x)
        if self.task_level != "graph":
            return x
        size = getattr(batch, "num_graphs", None)
        return global_mean_pool(x, batch_vec, size)                         # scatter_mean(x, batch, dim=0)


def build_mpnn(model_cfg: MPNNConfig, num_features: int, num_classes: int) -> MPNN:  # mpnn.py:65-78
    return MPNN(CONV_DICT[model_cfg.conv_type.lower()], ACT_DICT[model_cfg.activation.lower()], num_features,
                model_cfg.hidden_channels, num_classes, model_cfg.num_layers, model_cfg.dropout,
                model_cfg.use_batch_norm, model_cfg.use_layer_norm, getattr(model_cfg, "task_level", "graph"),
                getattr(model_cfg, "node_encoder", None), getattr(model_cfg, "edge_encoder", None),
                getattr(model_cfg, "heads", 1), getattr(model_cfg, "pos_enc", None),
                getattr(model_cfg, "pe_undirected", True), getattr(model_cfg, "pna", None))
