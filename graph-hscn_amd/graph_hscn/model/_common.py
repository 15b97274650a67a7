"""What the models spell alike, stated once: the validation of ``task_level`` (every model) and of the categorical
encoders' names, the float ``edge_attr`` check, the trainable positional encoder (``PosEnc``) and the link-level
``forward`` / ``embed`` pair (``LinkLevel``) of the homogeneous models, and ``LayeredModel``: the base of the
homogeneous models that run on the layered operators only (model/gps.py GPS, model/san.py SAN, model/gcnii.py GCNII) --
their construction steps, the surface ``train.batching`` and ``train.train`` use, the graph-level mean pool and the
head.  A further model of that kind subclasses it and writes its own arguments, its layer stack and ``_nodes``."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..config.config import ACT_DICT
from ..encoder.categorical import EDGE_ENCODERS, NODE_ENCODERS, resident_reason as encoder_reason
from ..nn import functional as Fh
from ..nn.conv import Linear
from ..nn.head import NodeHead
from ..nn.pool import global_mean_pool

# hscn_segment_mean_fwd (csrc/pool.hip) gives a row at most 64 lanes of four columns
POOL_MAX_WIDTH = 256


def check_task_level(task_level) -> None:
    if task_level not in ("graph", "node", "link"):
        raise ValueError(f"task_level must be 'graph', 'node' or 'link', not {task_level!r}")


def check_encoders(node_encoder, edge_encoder) -> None:
    if node_encoder not in (None,) + tuple(NODE_ENCODERS):
        raise ValueError(f"node_encoder must be one of {sorted(NODE_ENCODERS)} or None, not {node_encoder!r}")
    if edge_encoder not in (None,) + tuple(EDGE_ENCODERS):
        raise ValueError(f"edge_encoder must be one of {sorted(EDGE_ENCODERS)} or None, not {edge_encoder!r}")


def float_edge_attr(ea: Tensor, dev) -> Tensor:
    """``batch.edge_attr`` of a model without an edge encoder: float32 on the model's device, or a TypeError."""
    if ea.dtype != torch.float32 or ea.device != dev:
        raise TypeError(f"edge_attr must be float32 on the model's device ({dev}); got {ea.dtype} on "
                        f"{ea.device} (train.batching.to_device casts integer bond features)")
    return ea


POSENC_RESIDENT_REASON = ("a positional encoder inside the model (pos_enc: the LapPE / RWSE node encoder is trained with "
                          "the model and its statistics are computed per batch) has no one-launch, resident or captured "
                          "form; the model runs on the layered operators")
# bits of ``lap_eig_flag`` / ``rwse_flag`` (transform/posenc.py, transform/rwse.py)
_PE_FLAG_BITS = ((1, "a graph reached the eigensolver's sweep cap without converging"),
                 (2, "an edge with an end outside its graph"),
                 (4, "a graph beyond the batch's max_nodes"))


class PosEnc:
    """Mixin of a homogeneous model that owns a trainable positional encoder: ``pos_enc`` is a ``config.LapPEConfig``
    or ``config.RWSEConfig`` (or None: no encoder, nothing changes), the model's node encoder is built
    ``pos_enc.dim_pe`` columns narrower (``_pe_width``) and ``encode_nodes`` appends the encoder's columns:
    ``[h | pe]`` of the hidden width.  ``_init_pos_enc`` validates and records the config before the model's
    parameters are created; ``_build_pos_encoder`` creates ``pe_encoder`` and is called AFTER every parameter the
    model had before, so a model without ``pos_enc`` keeps its ``state_dict`` order and its RNG draws."""

    def _init_pos_enc(self, pos_enc, pe_undirected: bool, hidden: int) -> int:
        """Records the config; returns the width left for the node encoder (``hidden - dim_pe``; ``hidden`` without)."""
        from ..config.config import LapPEConfig, RWSEConfig
        self.pos_enc, self.pe_undirected = pos_enc, bool(pe_undirected)
        self._pe_flags = []                         # (kind, [1] int32 device tensor) of statistics not yet checked
        if pos_enc is None:
            return int(hidden)
        if not isinstance(pos_enc, (LapPEConfig, RWSEConfig)):
            raise ValueError(f"pos_enc must be a LapPEConfig, an RWSEConfig or None, not {type(pos_enc).__name__}")
        if int(pos_enc.dim_emb) != int(hidden):
            raise ValueError(f"pos_enc.dim_emb ({pos_enc.dim_emb}) must equal the model's hidden width ({hidden})")
        self.layered_only = True                    # train.batching.refuse_layered_only
        return int(hidden) - int(pos_enc.dim_pe)

    def _build_pos_encoder(self, hidden: int) -> None:
        from ..config.config import LapPEConfig
        if self.pos_enc is None:
            return
        if isinstance(self.pos_enc, LapPEConfig):
            from ..encoder.lappe import LapPENodeEncoder
            self.pe_encoder = LapPENodeEncoder(self.pos_enc, 1, int(hidden), expand_x=False)
        else:
            from ..encoder.rwse import RWSENodeEncoder
            self.pe_encoder = RWSENodeEncoder(self.pos_enc, 1, int(hidden), expand_x=False)

    def _pe_stats(self, batch):
        """The statistics ``pe_encoder`` reads: the batch's own where it carries them at the configured width, else
        computed ONCE per batch object on the model's device and kept in the dict ``train.batching._carry_host_side``
        hands from a loader's batch to its device copies, keyed by (kind, the settings that determine them, device).
        Nothing is read back: the launch's flag word waits for ``check_flags``."""
        from ..config.config import LapPEConfig
        cfg = self.pos_enc
        dev = str(batch.edge_index.device)
        cache = getattr(batch, "__dict__", {}).setdefault("_spd_cache", {})
        if isinstance(cfg, LapPEConfig):
            vec, val = getattr(batch, "eigvecs_sn", None), getattr(batch, "eigvals_sn", None)
            if vec is not None and val is not None and vec.dim() == 2 and vec.size(1) == cfg.eigen_max_freqs:
                return vec, val
            key = ("lappe", (int(cfg.eigen_max_freqs), cfg.eigvec_norm, cfg.eigen_laplacian_norm.lower(),
                             self.pe_undirected), dev)
            if key not in cache:
                from ..transform.posenc import _lap_eig_launch
                out, flag, _ = _lap_eig_launch(batch, self.pe_undirected, cfg)
                self._pe_flags.append(("lap_eig_flag", flag))
                cache[key] = (out[1], out[0])
            return cache[key]
        rw = getattr(batch, "rwse", None)
        if rw is not None and rw.dim() == 2 and rw.size(1) == cfg.ksteps:
            return (rw,)
        key = ("rwse", (int(cfg.ksteps), self.pe_undirected), dev)
        if key not in cache:
            from ..transform.rwse import _rwse_launch
            rw, flag = _rwse_launch(batch, self.pe_undirected, cfg)
            self._pe_flags.append(("rwse_flag", flag))
            cache[key] = (rw,)
        return cache[key]

    def _check_pe_flags(self) -> None:
        """Synchronising: raises for a nonzero flag word of any statistics computed since the last check."""
        if not getattr(self, "_pe_flags", None):
            return
        flags, self._pe_flags = self._pe_flags, []
        words = torch.cat([f for _, f in flags]).tolist()
        for (kind, _), w in zip(flags, words):
            if w:
                what = "; ".join(text for bit, text in _PE_FLAG_BITS if w & bit)
                raise RuntimeError(f"the positional encoder's statistics reported {kind} = {w}: {what}")

    def _embed_x(self, batch) -> Tensor:
        raise NotImplementedError

    def encode_nodes(self, batch) -> Tensor:
        """[N, D]: the node encoder's columns, and behind them the positional encoder's ``dim_pe`` where the model has
        one."""
        h = self._embed_x(batch)
        if self.pos_enc is None:
            return h
        return torch.cat((h, self.pe_encoder.pe(*self._pe_stats(batch))), 1)


class LinkLevel:
    """Mixin of a homogeneous model with ``task_level`` and ``_forward(batch)``: at "link" level ``_forward`` gives the
    [N, D] node embeddings, ``forward`` scores the batch's candidate pairs with them and ``embed`` hands them out."""

    def forward(self, batch) -> Tensor:
        out = self._forward(batch)
        if self.task_level == "link":                  # one score per candidate pair of the batch
            from ..nn.head import PairStructure, pair_dot
            return pair_dot(out, batch.edge_label_index, PairStructure.of(batch, out.size(0)))
        return out

    def embed(self, batch) -> Tensor:
        """The [N, D] node embeddings a link-level model scores pairs with: the node-level model's forward."""
        if self.task_level != "link":
            raise RuntimeError("embed() belongs to a link-level model (task_level='link')")
        return self._forward(batch)


class _Table(nn.Module):
    """A learned table ``weight`` [rows, D], drawn normal(0, 1) as an ``nn.Embedding`` is."""

    def __init__(self, rows: int, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(rows, channels))
        nn.init.normal_(self.weight)


class LayeredModel(LinkLevel, PosEnc, nn.Module):
    """A homogeneous model that runs on the layered operators only: a node encoder (Linear or "atom", with ``pos_enc``
    beside it), a stack ``layers`` of the subclass's own and one head per task level -- "graph": mean pool, ``Linear(D,
    D)``, activation, ``Linear(D, C)``; "node": the two Linears per node, through ``nn.head.NodeHead`` where its kernels
    apply; "link": the node level's output as embeddings (``LinkLevel``).

    A subclass's ``__init__`` calls the construction steps below in the order its ``state_dict`` and its RNG draws
    ask for -- ``_check_args``, its own checks, ``_record``, ``_build_node_encoder``, its layers and encoders,
    ``_build_head``, whatever it creates behind the head, ``_build_pos_encoder`` last -- and it writes ``_nodes`` and
    ``_own_reason``, and ``_check_launch_flags`` / ``_edge_attr_reader`` where it has launch flags / reads
    ``edge_attr``."""
    layered_only = True      # train.batching.refuse_layered_only: the resident entry points refuse the model by name

    # ---- construction steps ------------------------------------------------------------------------------------------
    def _check_args(self, node_encoder, edge_encoder, task_level, num_layers) -> None:
        check_encoders(node_encoder, edge_encoder)
        check_task_level(task_level)
        if num_layers < 1:
            raise ValueError(f"{type(self).__name__} needs at least one layer")

    def _record(self, task_level, num_layers, activation, dropout, node_encoder, edge_encoder) -> None:
        """Validates ``activation`` (None: ReLU) and records what every such model keeps."""
        activation = ACT_DICT["relu"] if activation is None else activation
        if getattr(activation, "hscn_name", None) is None:
            raise ValueError("activation must be one of config.ACT_DICT's (it runs in a Linear's epilogue)")
        self.task_level = task_level
        self.num_layers = int(num_layers)
        self.activation = activation
        self.dropout = float(dropout)
        self.dropout_seed: Optional[int] = None     # tests pin the masks (the subclass numbers its layers' seeds)
        self.encoder_kinds = (node_encoder, edge_encoder)
        # "layered"; "auto" runs layered too; "resident" raises with the reason when the model is called
        self.engine = "layered"
        self.last_engine: Optional[str] = None

    def _build_node_encoder(self, num_features, hidden, pos_enc, pe_undirected) -> None:
        width = self._init_pos_enc(pos_enc, pe_undirected, hidden)     # hidden - dim_pe with a positional encoder
        kind = self.encoder_kinds[0]
        self.node_encoder = Linear(num_features, width) if kind is None else NODE_ENCODERS[kind](width)

    def _build_head(self, hidden, num_classes) -> None:
        self.lin_1 = Linear(hidden, hidden)
        self.lin_2 = Linear(hidden, num_classes)
        self._node_head = NodeHead(self.lin_1, self.lin_2, self.activation.hscn_name)

    # ---- what a subclass supplies ------------------------------------------------------------------------------------
    def _own_reason(self) -> str:
        """Why the model's own layers have no one-launch, resident or captured form."""
        raise NotImplementedError

    def _check_launch_flags(self, dev) -> None:
        """The ``nn.functional.check_*`` of the flag words the model's own launches write (none by default)."""

    def _edge_attr_reader(self) -> str:
        """The opening of the missing-``edge_attr`` message: what in the model reads the edge features."""
        raise NotImplementedError

    def _nodes(self, batch) -> Tensor:
        """[N, D] after the last layer."""
        raise NotImplementedError

    # ---- the surface of a homogeneous model (train.batching, train.train) --------------------------------------------
    def resident_reason(self, batch=None, need_grad: bool = False) -> str:
        reason = self._own_reason()
        if self.pos_enc is not None:
            reason = reason + "; " + POSENC_RESIDENT_REASON
        if any(self.encoder_kinds):
            reason = reason + "; " + encoder_reason(*self.encoder_kinds)
        return reason

    def supported(self, batch=None) -> bool:
        return False

    def head_width(self) -> int:
        """Columns of the prediction (what ``batching.score_width`` asks for class-index targets)."""
        return int(self.lin_2.out_channels)

    def check_flags(self) -> None:
        """Synchronising: raises for a nonzero flag word of a launch since the last check -- the model's own
        (``_check_launch_flags``), the categorical encoders' (an index outside its column) and the positional encoder's
        statistics launches'.  ``train.train_epoch`` / ``eval_epoch`` call it once per epoch, beside the read of the
        epoch's loss."""
        dev = next(self.parameters()).device
        self._check_launch_flags(dev)
        if any(self.encoder_kinds):
            Fh.check_categorical(dev)
        self._check_pe_flags()

    # ---- forward -----------------------------------------------------------------------------------------------------
    def _edge_attr(self, batch) -> Tensor:
        """``batch.edge_attr`` as the model's edge encoder or layers read it: int64 categories for a categorical edge
        encoder (which checks them itself), else float32 [E, De] on the model's device."""
        ea = getattr(batch, "edge_attr", None)
        if ea is None:
            raise ValueError(f"{self._edge_attr_reader()} and the batch carries no edge_attr "
                             "(Data(edge_attr=[E, De]); make_dataset(..., edge_features=True))")
        if self.encoder_kinds[1] is not None:
            return ea
        return float_edge_attr(ea, next(self.parameters()).device)

    def _embed_x(self, batch) -> Tensor:
        return self.node_encoder(batch.x)

    def _pool(self, x: Tensor, batch) -> Tensor:
        """[B, D] graph means.  The mean pool's kernel takes ``POOL_MAX_WIDTH`` columns: a wider x (300, the LRGB
        width) is pooled in column slices of that many, a column's mean being the same sum either way."""
        num_graphs = getattr(batch, "num_graphs", None)
        if x.size(1) <= POOL_MAX_WIDTH:
            return global_mean_pool(x, batch.batch, num_graphs)
        parts = [global_mean_pool(x[:, c:c + POOL_MAX_WIDTH].contiguous(), batch.batch, num_graphs)
                 for c in range(0, x.size(1), POOL_MAX_WIDTH)]
        return torch.cat(parts, 1)

    def _head(self, x: Tensor) -> Tensor:
        h = Fh.linear_wide(x, self.lin_1.weight, self.lin_1.bias, self.activation.hscn_name)
        return Fh.linear_wide(h, self.lin_2.weight, self.lin_2.bias)

    def _forward(self, batch) -> Tensor:
        if self.engine not in ("layered", "auto", "resident"):
            raise ValueError(f"engine must be 'layered', 'auto' or 'resident', got {self.engine!r}")
        if self.engine == "resident":
            raise RuntimeError(f"engine='resident' does not take this model: {self.resident_reason()}")
        self.last_engine = "layered"
        x = self._nodes(batch)
        if self.task_level == "graph":
            return self._head(self._pool(x, batch))
        return self._node_head(x) if self._node_head.supported() else self._head(x)
