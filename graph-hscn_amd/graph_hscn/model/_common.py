"""What the models spell alike, stated once: the validation of ``task_level`` (MPNN, GPS, HSCN) and of the categorical
encoders' names, the float ``edge_attr`` check and the link-level ``forward`` / ``embed`` pair of the two homogeneous
models (model/mpnn.py MPNN, model/gps.py GPS)."""
from __future__ import annotations

import torch
from torch import Tensor

from ..encoder.categorical import EDGE_ENCODERS, NODE_ENCODERS


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
