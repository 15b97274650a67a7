"""Categorical input encoders: OGB's ``AtomEncoder`` / ``BondEncoder`` (ogb.graphproppred.mol_encoder), the input layer
of every LRGB Peptides baseline.  An integer feature tensor [n, F] becomes ``sum_c table_c[x[:, c]]``, the adds in
column order.  The F tables live in ONE ``weight [R, D]`` (column c owns rows ``offsets[c] .. offsets[c + 1] - 1``) so
that the forward is one gather launch and the backward one ordered segment reduce (csrc/catenc.hip): no float atomics,
bitwise reproducible -- carbon and the single bond collect a large share of every batch, which is the case atomics
handle worst.  ``to_ogb_state_dict`` / ``load_ogb_state_dict`` exchange weights with OGB's per-column tables."""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from ..nn import functional as Fh

# ogb.utils.features.get_atom_feature_dims() / get_bond_feature_dims(): what loader.synthetic draws its columns with
ATOM_FEATURE_DIMS = (119, 5, 12, 12, 10, 6, 6, 2, 2)
BOND_FEATURE_DIMS = (5, 6, 2)


class CategoricalEncoder(nn.Module):
    ogb_prefix = "embedding_list"

    def __init__(self, cardinalities: Sequence[int], emb_dim: int) -> None:
        super().__init__()
        cards = tuple(int(c) for c in cardinalities)
        if not cards or any(c < 1 for c in cards):
            raise ValueError(f"cardinalities must be a non-empty list of positive sizes, got {list(cardinalities)}")
        self.cardinalities = cards
        self.emb_dim = int(emb_dim)
        R = sum(cards)
        if not Fh.catenc_supported(self.emb_dim, len(cards), R):
            raise ValueError(f"emb_dim={emb_dim}, {len(cards)} columns, {R} categories: outside the kernel's envelope "
                             f"({Fh.CATENC_ENVELOPE})")
        self.offsets = tuple(sum(cards[:c]) for c in range(len(cards) + 1))
        self.weight = nn.Parameter(torch.empty(R, self.emb_dim))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            for c in range(len(self.cardinalities)):      # OGB: xavier_uniform_ on every table by itself
                nn.init.xavier_uniform_(self.weight[self.offsets[c]:self.offsets[c + 1]])

    def forward(self, x: Tensor) -> Tensor:
        if x.is_floating_point() or x.dtype == torch.bool:
            raise TypeError(f"{type(self).__name__} reads integer categories, got {x.dtype}: train.batching.to_device "
                            "keeps the features an encoder model reads as int64 (it casts them to float for a model "
                            "without one)")
        if x.dim() != 2 or x.size(1) != len(self.cardinalities):
            raise ValueError(f"{type(self).__name__} takes [n, {len(self.cardinalities)}] categories, got {tuple(x.shape)}")
        if x.dtype != torch.int64:
            x = x.long()
        if not x.is_contiguous():
            x = x.contiguous()
        return Fh.categorical_embed(self.weight, x, self.cardinalities)

    # ---- OGB's per-column tables -----------------------------------------------------------------------------------
    def to_ogb_state_dict(self) -> Dict[str, Tensor]:
        return {f"{self.ogb_prefix}.{c}.weight": self.weight.detach()[self.offsets[c]:self.offsets[c + 1]].clone()
                for c in range(len(self.cardinalities))}

    def load_ogb_state_dict(self, state: Dict[str, Tensor]) -> None:
        keys = [f"{self.ogb_prefix}.{c}.weight" for c in range(len(self.cardinalities))]
        if sorted(state) != sorted(keys):
            raise KeyError(f"expected the keys {keys}, got {sorted(state)}")
        for c, k in enumerate(keys):
            want = (self.cardinalities[c], self.emb_dim)
            if tuple(state[k].shape) != want:
                raise ValueError(f"{k} is {tuple(state[k].shape)}, the encoder's column is {want}")
        with torch.no_grad():
            for c, k in enumerate(keys):
                self.weight[self.offsets[c]:self.offsets[c + 1]].copy_(state[k])

    def extra_repr(self) -> str:
        return f"cardinalities={list(self.cardinalities)}, emb_dim={self.emb_dim}"


class AtomEncoder(CategoricalEncoder):
    ogb_prefix = "atom_embedding_list"

    def __init__(self, emb_dim: int) -> None:
        super().__init__(ATOM_FEATURE_DIMS, emb_dim)


class BondEncoder(CategoricalEncoder):
    ogb_prefix = "bond_embedding_list"

    def __init__(self, emb_dim: int) -> None:
        super().__init__(BOND_FEATURE_DIMS, emb_dim)


NODE_ENCODERS = {"atom": AtomEncoder}
EDGE_ENCODERS = {"bond": BondEncoder}
RESIDENT_REASON = ("a categorical input encoder ({what}): the one-launch, resident and device-dataset paths collate "
                   "float features; an encoder model reads int64 categories and runs on the layered operators")


def resident_reason(node_encoder, edge_encoder) -> str:
    what = ", ".join(f"{k}={v!r}" for k, v in (("node_encoder", node_encoder), ("edge_encoder", edge_encoder)) if v)
    return RESIDENT_REASON.format(what=what)
