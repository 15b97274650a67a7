"""Registries and config records with the reference's names and fields
(graph_hscn/config/config.py:13-152, defaults.py:1-39).

pydantic is not used: under the installed pydantic 2.x the reference's
``@root_validator`` raises at class creation, and wandb
is optional here (the reference makes it mandatory, config.py:146-152).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional

from torch.optim import Adagrad, Adam, AdamW

from ..nn.conv import GINE, PNA, EdgeTransformerConv, GATConv, GatedGCNConv, GCNConv, PNAEdge, TransformerConv
from ..nn.functional import Activation

# defaults.py:1-39
BATCH_SIZE = 32
NUM_WORKERS = 0
NUM_LAYERS = 3
HIDDEN_CHANNELS = 16
BATCH_ACCUMULATION = 1
CLIP_GRAD_NORM = False
LR = 0.01
WEIGHT_DECAY = 5e-4
EPOCHS = 500
EVAL_PERIOD = 10
MIN_DELTA = 0.01
PATIENCE = 2
NUM_CLUSTERS = 4
CLUSTER_EPOCHS = 10

ACT_DICT: dict[str, Callable] = {  # config.py:13-18
    "elu": Activation("elu"),
    "relu": Activation("relu"),
    "tanh": Activation("tanh"),
    "identity": Activation("identity"),
}
# config.py:19-23 also lists "gin": GINConv(dim, hidden, add_self_loops=...) raises a
# TypeError in PyG (GINConv takes an nn, not channel counts), so only gcn/gat can be
# built through build_conv_relation (model/hscn.py:117-125).  Both also build the MPNN baseline
# (model/mpnn.py:29-32 calls conv(in, out), i.e. add_self_loops=True): "gcn" through GCNConv's
# explicit-loop relation, "gat" through GATConv's shared transform and implicit-loop kernels
# (nn/conv.py, csrc/gat_loops.hip).  Only "gcn" qualifies for the one-launch MPNN step.
# "gine" (extension; "gin" stays absent, as it cannot be built in the reference either): the edge-aware baseline,
# nn/conv.py GINE = GINEConv over Linear-ReLU-Linear (csrc/gine.hip).  It reads ``batch.edge_attr``, builds the MPNN
# baseline only (the hetero graph carries no edge features: build_conv_relation refuses it) and runs layered.
# "gatedgcn" (extension): nn/conv.py GatedGCNConv (csrc/gatedgcn.hip), the edge-gated convolution whose edge features
# are a state: it reads ``batch.edge_attr``, returns ``(x, e)`` and hands ``e`` to the next layer.  Like "gine" it
# builds the MPNN baseline and the GPS local branch only, and runs layered.
# "transformerconv" / "transformerconv_edge" (extension): nn/conv.py TransformerConv / EdgeTransformerConv
# (csrc/edge_attention.hip), multi-head dot-product attention over the in-edges; the second adds ``batch.edge_attr`` to
# keys and values.  They take ``heads`` (MPNNConfig.heads, GPSConfig.num_heads, HSCNConfig.heads), run layered, and the
# first also builds HSCN's relations (build_conv_relation "TransformerConv").  The key is not "transformer": that name
# stays refused (GPS's plain Transformer layer is local_conv_type=None).
# "pna" / "pna_edge" (extension): nn/conv.py PNA / PNAEdge = PyG's PNAConv with one tower (csrc/pna.hip), several
# aggregators of the in-edge messages under degree scalers; the second feeds ``batch.edge_attr`` through its
# ``edge_encoder`` into the messages.  Which aggregators and scalers, and the training set's ``avg_deg_log``, come from
# a ``PNAConfig`` (MPNNConfig.pna / GPSConfig.pna; None: mean, min, max, std under the identity scaler).  They build the
# MPNN baseline and the GPS local branch, run layered, and HSCN's relations do not take them yet.
CONV_DICT: dict[str, type] = {"gcn": GCNConv, "gat": GATConv, "gine": GINE, "gatedgcn": GatedGCNConv,
                              "transformerconv": TransformerConv, "transformerconv_edge": EdgeTransformerConv,
                              "pna": PNA, "pna_edge": PNAEdge}
# conv_type whose layers are built with ``heads``
MULTI_HEAD_CONVS = ("transformerconv", "transformerconv_edge")
OPTIM_DICT: dict[str, type] = {"adagrad": Adagrad, "adam": Adam, "adamW": AdamW}  # config.py:24-28
SCHEDULERS = ("cosine_with_warmup", "linear_with_warmup", "step")  # extension: optim.SCHEDULE_KINDS
TASK_LEVELS = ("graph", "node", "link")  # extension: the reference serves "graph" only
# extension: categorical input encoders in front of a model (encoder/categorical.py: OGB's AtomEncoder / BondEncoder)
NODE_ENCODERS = ("atom",)
EDGE_ENCODERS = ("bond",)
# conv_type / local_conv_type whose layers read ``edge_attr`` (nn/conv.py ``uses_edge_attr``): what an edge encoder feeds
EDGE_AWARE_CONVS = ("gine", "gatedgcn", "transformerconv_edge", "pna_edge")
# conv_type / local_conv_type whose layers are built from a PNAConfig
PNA_CONVS = ("pna", "pna_edge")


GPS_NORMS = ("layer", "batch", None)


def _check_task_level(task_level) -> None:
    if task_level not in TASK_LEVELS:
        raise ValueError(f"task_level must be 'graph', 'node' or 'link', got {task_level!r}")


def _check_activation(activation) -> None:
    if activation.lower() not in ACT_DICT:
        raise ValueError(f"activation must be one of {sorted(ACT_DICT)}, got {activation!r}")


def _check_encoder_names(node_encoder, edge_encoder=None) -> None:
    """The names alone: SAN and GCNII have no ``conv_type`` to tie an edge encoder to (``_check_encoders`` does)."""
    if node_encoder not in (None,) + NODE_ENCODERS:
        raise ValueError(f"node_encoder must be one of {NODE_ENCODERS} or None, got {node_encoder!r}")
    if edge_encoder not in (None,) + EDGE_ENCODERS:
        raise ValueError(f"edge_encoder must be one of {EDGE_ENCODERS} or None, got {edge_encoder!r}")


def _check_dropout(dropout) -> None:
    """[0, 1): the layered-only models' rule (MPNNConfig keeps the reference's, which admits 1.0)."""
    if dropout and not (0.0 <= dropout < 1.0):
        raise ValueError(f"{dropout} must be in [0.0, 1.0).")


def _check_positive(*values) -> None:
    for v in values:
        if v < 1:
            raise ValueError(f"{v} must be positive.")


def _check_norm(norm) -> None:
    if norm not in GPS_NORMS:
        raise ValueError(f"norm must be 'layer', 'batch' or None, got {norm!r}")


def _check_attention_width(hidden_channels, num_heads) -> None:
    """The envelope GPS's and SAN's attention kernels share (csrc/attention.hip, csrc/san.hip)."""
    if hidden_channels % num_heads:
        raise ValueError(f"hidden_channels {hidden_channels} must be divisible by num_heads {num_heads}.")
    dh = hidden_channels // num_heads
    if dh % 4 or not 4 <= dh <= 64 or hidden_channels > 512:
        raise ValueError(f"head width {dh} (hidden_channels / num_heads) must be a multiple of 4 in [4, 64] and "
                         f"hidden_channels at most 512.")


def check_exphormer(expander_degree, num_virtual_nodes) -> None:
    """Exphormer's two sizes against the kernels' bounds: what ``GPSConfig`` and ``model.gps.GPS`` both ask."""
    from ..nn.functional import EXPANDER_MAX_DEGREE, EXPH_MAX_VIRTUAL_NODES
    d, nv = expander_degree, num_virtual_nodes
    if isinstance(d, bool) or not isinstance(d, int) or d % 2 or not 2 <= d <= EXPANDER_MAX_DEGREE:
        raise ValueError(f"expander_degree must be an even integer in [2, {EXPANDER_MAX_DEGREE}], got {d!r}")
    if isinstance(nv, bool) or not isinstance(nv, int) or not 0 <= nv <= EXPH_MAX_VIRTUAL_NODES:
        raise ValueError(f"num_virtual_nodes must be an integer in [0, {EXPH_MAX_VIRTUAL_NODES}], got {nv!r}")


def _check_encoders(node_encoder, edge_encoder, conv_type) -> None:
    _check_encoder_names(node_encoder, edge_encoder)
    if edge_encoder is not None and (conv_type is None or conv_type.lower() not in EDGE_AWARE_CONVS):
        raise ValueError(f"edge_encoder={edge_encoder!r} needs an edge-aware convolution {EDGE_AWARE_CONVS}, "
                         f"got {conv_type!r}")


def _check_pos_enc(pos_enc, hidden_channels) -> None:
    if pos_enc is None:
        return
    if not isinstance(pos_enc, (LapPEConfig, RWSEConfig)):
        raise ValueError(f"pos_enc must be a LapPEConfig, an RWSEConfig or None, got {type(pos_enc).__name__}")
    if pos_enc.dim_emb != hidden_channels:
        raise ValueError(f"pos_enc.dim_emb ({pos_enc.dim_emb}) must equal hidden_channels ({hidden_channels})")


def check_heads(heads, hidden_channels, conv_type) -> None:
    if not isinstance(heads, int) or heads < 1:
        raise ValueError(f"heads must be a positive int, got {heads!r}")
    if heads != 1 and (conv_type is None or conv_type.lower() not in MULTI_HEAD_CONVS):
        raise ValueError(f"heads={heads} needs a multi-head convolution {MULTI_HEAD_CONVS}, got {conv_type!r}")
    if hidden_channels % heads:
        raise ValueError(f"hidden_channels {hidden_channels} must be divisible by heads {heads}.")


@dataclass
class PNAConfig:
    """What the "pna" / "pna_edge" layers of a model are built with (nn/conv.py PNAConv): ``aggregators`` out of mean,
    min, max, sum, std; ``scalers`` out of identity, amplification, attenuation; ``avg_deg_log``, the training set's mean
    of ``log(in-degree + 1)``, required beside a scaler other than identity (``from_graphs`` computes it)."""
    aggregators: tuple = ("mean", "min", "max", "std")
    scalers: tuple = ("identity",)
    avg_deg_log: Optional[float] = None

    def __post_init__(self) -> None:
        from ..nn.functional import pna_codes
        for name in ("aggregators", "scalers"):
            v = getattr(self, name)
            if isinstance(v, str) or not isinstance(v, (tuple, list)):
                raise ValueError(f"{name} must be a tuple of names, got {v!r}")
            setattr(self, name, tuple(v))
        for s in self.scalers:
            if s in ("linear", "inverse_linear"):
                raise ValueError(f"the scaler {s!r} is not provided (identity, amplification, attenuation are)")
        pna_codes(self.aggregators, self.scalers)
        a = self.avg_deg_log
        if a is not None and (isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 < float(a) < float("inf")):
            raise ValueError(f"avg_deg_log must be a positive, finite number or None, got {a!r}")
        if a is None and any(s != "identity" for s in self.scalers):
            raise ValueError(f"scalers {self.scalers} need avg_deg_log (PNAConfig.from_graphs computes it from the "
                             "training graphs)")

    @staticmethod
    def avg_deg_log_of(graphs) -> float:
        """The mean of ``log(in-degree + 1)`` over every node of ``graphs`` (``Data`` with ``edge_index`` and
        ``num_nodes``): PyG's ``avg_deg['log']`` of the training set, on the host in float64."""
        import torch
        total, nodes = 0.0, 0
        for g in graphs:
            n = int(g.num_nodes)
            deg = torch.bincount(g.edge_index[1].cpu(), minlength=n).to(torch.float64)
            total += float(torch.log(deg + 1.0).sum())
            nodes += n
        if nodes == 0:
            raise ValueError("avg_deg_log needs at least one node")
        return total / nodes

    @classmethod
    def from_graphs(cls, graphs, aggregators=("mean", "min", "max", "std"),
                    scalers=("identity", "amplification", "attenuation")) -> "PNAConfig":
        return cls(tuple(aggregators), tuple(scalers), cls.avg_deg_log_of(graphs))


def pna_kwargs(pna: Optional[PNAConfig]) -> dict:
    """The keywords a "pna" / "pna_edge" layer is built with (None: the layer's defaults)."""
    return {} if pna is None else dict(aggregators=pna.aggregators, scalers=pna.scalers, avg_deg_log=pna.avg_deg_log)


def _check_pna(pna, conv_type) -> None:
    if pna is None:
        return
    if not isinstance(pna, PNAConfig):
        raise ValueError(f"pna must be a PNAConfig or None, got {type(pna).__name__}")
    if conv_type is None or conv_type.lower() not in PNA_CONVS:
        raise ValueError(f"pna=PNAConfig(...) needs a PNA convolution {PNA_CONVS}, got {conv_type!r}")


DATASETS_NUM_FEATURES: dict[str, int] = {"peptides_func": 9, "peptides_struct": 9}


@dataclass
class DataConfig:  # config.py:32-46
    dataset_name: str
    pe: bool = False
    batch_size: int = BATCH_SIZE
    num_workers: int = NUM_WORKERS
    task_level: Optional[str] = None

    def __post_init__(self):
        self.task_level = "graph" if "peptides" in self.dataset_name else (self.task_level or "graph")


DROPOUT = 0.2  # defaults.py:6
USE_BATCH_NORM = False
USE_LAYER_NORM = False


@dataclass
class MPNNConfig:  # config.py:49-73
    conv_type: str
    activation: str
    hidden_channels: int = HIDDEN_CHANNELS
    num_layers: int = NUM_LAYERS
    dropout: float = DROPOUT
    use_batch_norm: bool = USE_BATCH_NORM
    use_layer_norm: bool = USE_LAYER_NORM
    # extension: "node" = one prediction per node (model/mpnn.py MPNN(task_level="node")); "link" = one score per
    # candidate pair of nodes, num_classes being the embedding width; "graph": the reference
    task_level: str = "graph"
    # extension: "atom" = an AtomEncoder(hidden_channels) in front (x stays int64; the first convolution is H -> H);
    # "bond" = a BondEncoder(hidden_channels) whose output the edge-aware convolutions read as edge_attr
    node_encoder: Optional[str] = None
    edge_encoder: Optional[str] = None
    # extension: attention heads of conv_type "transformerconv" / "transformerconv_edge": the hidden layers are
    # conv(in, hidden_channels // heads, heads=heads), the last one has one head of width num_classes
    heads: int = 1
    # extension: a trainable positional encoder inside the model (model/_common.py PosEnc): a LapPEConfig or an
    # RWSEConfig whose dim_emb is hidden_channels; pe_undirected: the edge lists hold both directions
    pos_enc: Optional[object] = None
    pe_undirected: bool = True
    # extension: aggregators, scalers and avg_deg_log of conv_type "pna" / "pna_edge" (None: PNAConfig's defaults)
    pna: Optional[PNAConfig] = None

    def __post_init__(self):
        _check_task_level(self.task_level)
        _check_encoders(self.node_encoder, self.edge_encoder, self.conv_type)
        _check_pna(self.pna, self.conv_type)
        _check_pos_enc(self.pos_enc, self.hidden_channels)
        check_heads(self.heads, self.hidden_channels, self.conv_type)
        if self.dropout and not (0.0 <= self.dropout <= 1.0):
            raise ValueError(f"{self.dropout} must be between 0.0 and 1.0.")
        for v in (self.num_layers, self.hidden_channels):
            if v < 0:
                raise ValueError(f"{v} must be non-negative.")


@dataclass
class GPSConfig:
    """The GPS model (extension; model/gps.py): ``num_layers`` GPS layers of width ``hidden_channels`` -- a local
    convolution ``local_conv_type`` ("gcn", "gat", "gine", "gatedgcn", "transformerconv", "transformerconv_edge", "pna",
    "pna_edge" of CONV_DICT, or None: the plain Transformer layer; "gatedgcn" is GraphGPS's published pairing: a ``GatedGCNLayer``
    that also updates the edge features; the two TransformerConv keys take ``num_heads`` heads as well) beside
    per-graph self-attention of ``num_heads`` heads, then a feed-forward block -- behind a Linear node encoder.  The
    head width ``hidden_channels / num_heads`` must be a multiple of 4 in [4, 64] and ``hidden_channels`` at most 512
    (the attention kernel's envelope, csrc/attention.hip)."""
    activation: str
    local_conv_type: Optional[str] = "gine"
    hidden_channels: int = HIDDEN_CHANNELS
    num_layers: int = NUM_LAYERS
    num_heads: int = 4
    dropout: float = DROPOUT
    norm: Optional[str] = "layer"
    task_level: str = "graph"
    # "atom" / "bond": an AtomEncoder / BondEncoder of width hidden_channels in place of the Linear node / edge encoder
    node_encoder: Optional[str] = None
    edge_encoder: Optional[str] = None
    # "spd": Graphormer's spatial encoding -- a learned bias per (shortest-path bucket, head) in every layer's attention,
    # distances of spd_max_dist hops and beyond (and unreachable pairs) sharing the last bucket
    attn_bias: Optional[str] = None
    spd_max_dist: int = 20
    # "exphormer": sparse attention over the batch's own edges (add_local_edges), a random expander of even degree
    # expander_degree drawn under expander_seed, and num_virtual_nodes virtual nodes per graph, in place of the dense
    # per-graph attention; the four further keys are read by "exphormer" only
    global_model: str = "attention"
    expander_degree: int = 6
    num_virtual_nodes: int = 1
    add_local_edges: bool = True
    expander_seed: int = 0
    # a trainable positional encoder inside the model (model/_common.py PosEnc): a LapPEConfig or an RWSEConfig whose
    # dim_emb is hidden_channels; pe_undirected: the edge lists hold both directions
    pos_enc: Optional[object] = None
    pe_undirected: bool = True
    # aggregators, scalers and avg_deg_log of local_conv_type "pna" / "pna_edge" (None: PNAConfig's defaults)
    pna: Optional[PNAConfig] = None

    def __post_init__(self):
        _check_task_level(self.task_level)
        _check_encoders(self.node_encoder, self.edge_encoder, self.local_conv_type)
        _check_pna(self.pna, self.local_conv_type)
        _check_pos_enc(self.pos_enc, self.hidden_channels)
        if self.attn_bias not in (None, "spd"):
            raise ValueError(f"attn_bias must be 'spd' or None, got {self.attn_bias!r}")
        if self.global_model not in ("attention", "exphormer"):
            raise ValueError(f"global_model must be 'attention' or 'exphormer', got {self.global_model!r}")
        if self.global_model == "exphormer" and self.attn_bias is not None:
            raise ValueError(f"global_model='exphormer' and attn_bias={self.attn_bias!r} do not go together: the "
                             "shortest-path bias belongs to the dense attention (attn_bias must be None)")
        check_exphormer(self.expander_degree, self.num_virtual_nodes)
        if not isinstance(self.add_local_edges, bool):
            raise ValueError(f"add_local_edges must be a bool, got {self.add_local_edges!r}")
        if isinstance(self.expander_seed, bool) or not isinstance(self.expander_seed, int) or self.expander_seed < 0:
            raise ValueError(f"expander_seed must be a non-negative integer, got {self.expander_seed!r}")
        if isinstance(self.spd_max_dist, bool) or not isinstance(self.spd_max_dist, int) or \
                not 1 <= self.spd_max_dist <= 63:
            raise ValueError(f"spd_max_dist must be an integer in [1, 63], got {self.spd_max_dist!r}")
        _check_dropout(self.dropout)
        _check_positive(self.num_layers, self.hidden_channels, self.num_heads)
        if self.local_conv_type is not None and self.local_conv_type.lower() not in CONV_DICT:
            raise ValueError(f"local_conv_type must be one of {sorted(CONV_DICT)} or None, got {self.local_conv_type!r}")
        _check_norm(self.norm)
        _check_attention_width(self.hidden_channels, self.num_heads)


@dataclass
class SANConfig:
    """The SAN model (extension; model/san.py): ``num_layers`` SAN layers of width ``hidden_channels`` -- attention of
    ``num_heads`` heads over every ordered pair of a graph, the listed edges ("real") through one set of projections
    and their encoded features, all other pairs ("fake") through a second set and one learned row, mixed by the fixed
    ``gamma`` >= 0 -- behind a node encoder (Linear or "atom") and an edge encoder (Linear or "bond").  The batches must
    carry ``edge_attr``.  ``full_graph=False`` keeps the real pairs alone.  The head width ``hidden_channels /
    num_heads`` must be a multiple of 4 in [4, 64] and ``hidden_channels`` at most 512 (the kernel's envelope,
    csrc/san.hip).  ``activation`` is the head's; the layers' feed-forward block is ReLU.  A learned gamma and dropout on
    the attention weights are not built (``SAN(gamma_learn=...)`` / ``SAN(attn_dropout=...)`` refuse them by name)."""
    activation: str
    hidden_channels: int = HIDDEN_CHANNELS
    num_layers: int = NUM_LAYERS
    num_heads: int = 4
    dropout: float = DROPOUT
    norm: Optional[str] = "layer"
    task_level: str = "graph"
    node_encoder: Optional[str] = None
    edge_encoder: Optional[str] = None
    gamma: float = 1e-1
    full_graph: bool = True
    # a trainable positional encoder inside the model (model/_common.py PosEnc): a LapPEConfig or an RWSEConfig whose
    # dim_emb is hidden_channels; pe_undirected: the edge lists hold both directions
    pos_enc: Optional[object] = None
    pe_undirected: bool = True

    def __post_init__(self):
        _check_task_level(self.task_level)
        _check_activation(self.activation)
        _check_encoder_names(self.node_encoder, self.edge_encoder)
        _check_pos_enc(self.pos_enc, self.hidden_channels)
        g = self.gamma
        if isinstance(g, bool) or not isinstance(g, (int, float)) or not 0.0 <= float(g) < float("inf"):
            raise ValueError(f"gamma must be a finite number >= 0, got {g!r}")
        if not isinstance(self.full_graph, bool):
            raise ValueError(f"full_graph must be a bool, got {self.full_graph!r}")
        _check_dropout(self.dropout)
        _check_positive(self.num_layers, self.hidden_channels, self.num_heads)
        _check_norm(self.norm)
        _check_attention_width(self.hidden_channels, self.num_heads)


@dataclass
class GCNIIConfig:
    """The GCNII model (extension; model/gcnii.py, LRGB's GCNII baseline): ``num_layers`` ``GCN2Conv`` layers of width
    ``hidden_channels`` -- each reads the running representation and the encoder's output x_0, mixed by ``alpha``, through
    a weight whose share ``beta_l = log(theta / l + 1)`` decays with depth (``theta=None``: 1) -- with ReLU and dropout
    after each, ``residual`` adding the layer's input, behind a node encoder (Linear or "atom").  ``edge_attr`` is not
    read.  ``hidden_channels`` must be a multiple of 4 in [4, 512] (the kernel's envelope, csrc/gcn2.hip).
    ``activation`` is the head's."""
    activation: str
    hidden_channels: int = HIDDEN_CHANNELS
    num_layers: int = NUM_LAYERS
    dropout: float = DROPOUT
    alpha: float = 0.1
    theta: Optional[float] = 0.5
    shared_weights: bool = True
    residual: bool = False
    task_level: str = "graph"
    node_encoder: Optional[str] = None
    # a trainable positional encoder inside the model (model/_common.py PosEnc): a LapPEConfig or an RWSEConfig whose
    # dim_emb is hidden_channels; pe_undirected: the edge lists hold both directions
    pos_enc: Optional[object] = None
    pe_undirected: bool = True

    def __post_init__(self):
        from ..nn.functional import GCN2_ENVELOPE, gcn2_supported
        _check_task_level(self.task_level)
        _check_activation(self.activation)
        _check_encoder_names(self.node_encoder)
        _check_pos_enc(self.pos_enc, self.hidden_channels)
        a, t = self.alpha, self.theta
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 <= float(a) <= 1.0:
            raise ValueError(f"alpha must be a number in [0, 1], got {a!r}")
        if t is not None and (isinstance(t, bool) or not isinstance(t, (int, float))
                              or not 0.0 < float(t) < float("inf")):
            raise ValueError(f"theta must be a positive, finite number or None, got {t!r}")
        for name in ("shared_weights", "residual"):
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"{name} must be a bool, got {getattr(self, name)!r}")
        _check_dropout(self.dropout)
        if isinstance(self.num_layers, bool) or not isinstance(self.num_layers, int) or self.num_layers < 1:
            raise ValueError(f"num_layers must be an int >= 1, got {self.num_layers!r}")
        h = self.hidden_channels
        if isinstance(h, bool) or not isinstance(h, int) or not gcn2_supported(h):
            raise ValueError(f"hidden_channels = {h!r} outside the GCN2Conv kernel's envelope ({GCN2_ENVELOPE}).")
        if t is not None and math.log(float(t) + 1.0) > 1.0:
            raise ValueError(f"theta = {t!r} gives beta_1 = log(theta + 1) > 1; theta must be at most e - 1")


@dataclass
class HSCNConfig:  # config.py:76-93 (+ mp_units, read at main.py:102 but absent there)
    activation: str
    lv_conv_type: str = "GAT"
    ll_conv_type: str = "GCN"
    vv_conv_type: str = "GCN"
    hidden_channels: int = HIDDEN_CHANNELS
    num_layers: int = NUM_LAYERS
    num_clusters: int = NUM_CLUSTERS
    cluster_epochs: int = CLUSTER_EPOCHS
    mp_units: list = field(default_factory=lambda: [16])
    # extension (keyword-only, so the positional order above and below is what it was): "node" = one prediction per
    # local node (model/hscn.py HSCN(task_level="node")); "link" = one score per candidate pair of local nodes,
    # num_classes being the embedding width; "graph": the reference
    task_level: str = field(default="graph", kw_only=True)
    # extension: attention heads of the relations built as "TransformerConv" (model/hscn.py build_conv_relation)
    heads: int = field(default=1, kw_only=True)
    # extension: the ("virtual", "to", "local") relation the reference never wired up (None: the reference's model,
    # whose virtual branch does not reach the prediction; "GAT": model/hscn.py HSCN(vl_conv="GAT"))
    vl_conv_type: Optional[str] = None

    def __post_init__(self):
        _check_task_level(self.task_level)
        if not isinstance(self.heads, int) or self.heads < 1:
            raise ValueError(f"heads must be a positive int, got {self.heads!r}")
        convs = (self.lv_conv_type, self.ll_conv_type, self.vv_conv_type)
        if self.heads != 1 and not any(str(c).lower() == "transformerconv" for c in convs):
            raise ValueError(f"heads={self.heads} needs a relation built as 'TransformerConv', got {convs}")
        if self.hidden_channels % self.heads:
            raise ValueError(f"hidden_channels {self.hidden_channels} must be divisible by heads {self.heads}.")
        for v in (self.num_layers, self.hidden_channels):
            if v < 0:
                raise ValueError(f"{v} must be non-negative.")


@dataclass
class OptimConfig:  # config.py:96-112
    optim_type: str
    batch_accumulation: int = BATCH_ACCUMULATION
    clip_grad_norm: bool = CLIP_GRAD_NORM
    lr: float = LR
    weight_decay: float = WEIGHT_DECAY
    # extension: a learning-rate schedule evaluated inside the one-launch optimizer (optim.LRSchedule; None: the
    # reference's constant rate).  "cosine_with_warmup" / "linear_with_warmup": ``warmup_epochs`` of linear warm-up,
    # then down to ``min_lr_factor * lr`` at the last epoch; "step": ``lr *= gamma`` every ``step_epochs`` epochs.
    scheduler: Optional[str] = None
    warmup_epochs: int = 0
    step_epochs: int = 1
    gamma: float = 1.0
    min_lr_factor: float = 0.0

    def __post_init__(self):
        for v in (self.lr, self.weight_decay, self.gamma, self.min_lr_factor):
            if v and not (0.0 <= v <= 1.0):
                raise ValueError(f"{v} must be between 0.0 and 1.0.")
        if self.scheduler not in (None,) + SCHEDULERS:
            raise ValueError(f"scheduler must be one of {SCHEDULERS} or None, got {self.scheduler!r}")
        if self.warmup_epochs < 0:
            raise ValueError(f"{self.warmup_epochs} must be non-negative.")
        if self.step_epochs < 1:
            raise ValueError("step_epochs must be at least 1.")
        if not self.gamma > 0.0:
            raise ValueError("gamma must be in (0, 1].")


@dataclass
class PEConfig:  # config.py:115-130 (defaults.py:19-28)
    dim_in: int
    dim_emb: int
    dim_pe: int
    model: str = "DeepSet"
    layers: int = 1
    post_layers: int = 1
    eigen_max_freqs: int = 10
    eigvec_norm: str = "L2"
    eigen_laplacian_norm: str = "sym"
    phi_hidden_dim: int = 32
    phi_out_dim: int = 4
    pass_as_var: bool = False
    use_bn: bool = False


@dataclass
class RWSEConfig:
    """Random-walk structural encoding (transform/rwse.py, encoder/rwse.py): ``ksteps`` return probabilities per node,
    encoded to ``dim_pe`` columns by one Linear ("linear") or ``layers`` Linear + ReLU ("mlp"), optionally behind a
    BatchNorm over the raw statistics; ``compute_posenc`` dispatches on the config's type."""
    dim_in: int
    dim_emb: int
    dim_pe: int
    ksteps: int = 20
    model: str = "linear"
    layers: int = 1
    raw_norm: str = "none"
    pass_as_var: bool = False

    def __post_init__(self) -> None:
        if self.ksteps < 1:
            raise ValueError("ksteps must be at least 1.")
        if self.model not in ("linear", "mlp"):
            raise ValueError(f"model must be 'linear' or 'mlp', got {self.model!r}.")
        if self.layers < 1:
            raise ValueError("layers must be at least 1.")
        if self.raw_norm not in ("none", "batchnorm"):
            raise ValueError(f"raw_norm must be 'none' or 'batchnorm', got {self.raw_norm!r}.")
        if self.dim_emb - self.dim_pe < 1:
            raise ValueError(f"RWSE size {self.dim_pe} is too large for desired embedding size of {self.dim_emb}.")


@dataclass
class LapPEConfig:
    """Laplacian positional encoding, GraphGPS's ``LapPENodeEncoder`` with the DeepSet model (encoder/lappe.py,
    csrc/lappe.hip): per node the ``eigen_max_freqs`` (eigenvector entry, eigenvalue) pairs go through ``layers``
    Linear + ReLU (2 -> 2 dim_pe -> ... -> dim_pe), the frequencies that exist are summed and ``post_layers`` Linear +
    ReLU follow; in training mode ``sign_flip`` flips the sign of whole eigenvector columns at random.  The three
    eigen-settings are read by ``transform.compute_posenc_stats_device``; ``compute_posenc`` and the models' ``pos_enc``
    dispatch on the config's type."""
    dim_in: int
    dim_emb: int
    dim_pe: int
    model: str = "DeepSet"
    layers: int = 2
    post_layers: int = 0
    eigen_max_freqs: int = 10
    eigvec_norm: str = "L2"
    eigen_laplacian_norm: str = "none"
    raw_norm: str = "none"
    sign_flip: bool = True
    pass_as_var: bool = False

    def __post_init__(self) -> None:
        from ..nn.functional import LAPPE_ENVELOPE, lappe_supported
        if self.model == "Transformer":
            raise ValueError("model='Transformer' (the Transformer variant of the LapPE encoder) is not built; "
                             "model must be 'DeepSet'.")
        if self.model != "DeepSet":
            raise ValueError(f"model must be 'DeepSet', got {self.model!r}.")
        if self.raw_norm == "batchnorm":
            raise ValueError("raw_norm='batchnorm' is not built for the LapPE encoder (the fused operator reads the "
                             "raw statistics); raw_norm must be 'none'.")
        if self.raw_norm != "none":
            raise ValueError(f"raw_norm must be 'none', got {self.raw_norm!r}.")
        for name in ("eigen_max_freqs", "dim_pe", "layers", "post_layers"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"{name} must be an int, got {v!r}.")
        if not lappe_supported(self.eigen_max_freqs, self.dim_pe, self.layers):
            raise ValueError(f"eigen_max_freqs={self.eigen_max_freqs}, dim_pe={self.dim_pe}, layers={self.layers} "
                             f"outside the LapPE kernel's envelope ({LAPPE_ENVELOPE}).")
        if self.post_layers < 0:
            raise ValueError("post_layers must be non-negative.")
        if self.dim_emb - self.dim_pe < 1:
            raise ValueError(f"LapPE size {self.dim_pe} is too large for desired embedding size of {self.dim_emb}.")


@dataclass
class TrainingConfig:  # config.py:133-152
    # "hscn" / "mpnn" (the reference's two: HSCNConfig / MPNNConfig), "gps" (extension: GPSConfig, model/gps.py),
    # "san" (extension: SANConfig, model/san.py) or "gcnii" (extension: GCNIIConfig, model/gcnii.py)
    model_type: str
    loss_fn: str
    # "ap" / "mae" (the reference's two), "accuracy" / "f1_macro" for class-index targets, or "mrr" / "hits@1" /
    # "hits@3" / "hits@10" for a link-level model (graph_hscn.metrics)
    metric: str
    epochs: int = EPOCHS
    eval_period: int = EVAL_PERIOD
    min_delta: float = MIN_DELTA
    patience: int = PATIENCE
    use_wandb: bool = False
    wandb_proj_name: Optional[str] = None
