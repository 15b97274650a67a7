"""Node encoder of the Laplacian positional encoding, GraphGPS's ``LapPENodeEncoder`` with the DeepSet model: per node
the ``eigen_max_freqs`` pairs (eigenvector entry, eigenvalue) go through ``linear_A`` and the ``pe_encoder`` Linears --
``layers`` Linear + ReLU in all, 2 -> 2 dim_pe -> ... -> dim_pe -- the frequencies that exist (a NaN eigenvector entry
marks padding) are summed, ``post_mlp`` follows, and the ``dim_pe`` columns are appended to the (optionally expanded)
node features.  Chain and sum are ONE launch (``nn.functional.LapPEDeepSetFn``, csrc/lappe.hip): the per-(node,
frequency) activations never exist in memory.  In training mode, with ``cfg.sign_flip``, whole eigenvector columns
change sign at random (Philox under a host seed; the backward regenerates the signs)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..nn import Linear
from ..nn import functional as Fh


class LapPENodeEncoder(nn.Module):
    def __init__(self, cfg, dim_in: int, dim_emb: int, expand_x: bool = True) -> None:
        super().__init__()
        dim_pe, K, L = int(cfg.dim_pe), int(cfg.eigen_max_freqs), int(cfg.layers)
        if cfg.model != "DeepSet":
            raise ValueError(f"Unexpected LapPE model {cfg.model}: only 'DeepSet' is built")
        if getattr(cfg, "raw_norm", "none") != "none":
            raise ValueError(f"raw_norm={cfg.raw_norm!r} is not built for the LapPE encoder")
        if not Fh.lappe_supported(K, dim_pe, L):
            raise ValueError(f"eigen_max_freqs={K}, dim_pe={dim_pe}, layers={L} outside the LapPE kernel's envelope "
                             f"({Fh.LAPPE_ENVELOPE})")
        if dim_emb - dim_pe < 1:
            raise ValueError(f"LapPE size {dim_pe} is too large for desired embedding size of {dim_emb}.")
        self.max_freqs = K
        self.sign_flip = bool(getattr(cfg, "sign_flip", True))
        self.pass_as_var = cfg.pass_as_var
        self.expand_x = expand_x
        self.pe_seed: Optional[int] = None          # tests pin the flips; None = nn.functional.default_seed()
        widths = Fh.lappe_widths(dim_pe, L)
        self.linear_A = Linear(widths[0], widths[1])
        self.pe_encoder = nn.ModuleList(Linear(i, o) for i, o in zip(widths[1:-1], widths[2:]))
        post = int(getattr(cfg, "post_layers", 0))
        pw = [dim_pe] + [2 * dim_pe] * (post - 1) + [dim_pe] if post > 0 else [dim_pe]
        self.post_mlp = nn.ModuleList(Linear(i, o) for i, o in zip(pw[:-1], pw[1:]))
        if expand_x:
            self.linear_x = Linear(dim_in, dim_emb - dim_pe)

    def pe(self, vec: Tensor, val: Tensor) -> Tensor:
        """[N, dim_pe] from ``vec`` [N, K] and ``val`` [N, K] (or [N, K, 1], as the statistics carry it)."""
        if val.dim() == 3:
            val = val.squeeze(2)
        if vec.dim() != 2 or vec.size(1) != self.max_freqs or val.shape != vec.shape:
            raise ValueError(f"the Laplacian statistics must be [N, {self.max_freqs}] (eigen_max_freqs), got "
                             f"{tuple(vec.shape)} and {tuple(val.shape)}")
        seed = None
        if self.training and self.sign_flip:
            seed = Fh.default_seed() if self.pe_seed is None else int(self.pe_seed)
        chain = [self.linear_A] + list(self.pe_encoder)
        pe = Fh.LapPEDeepSetFn.apply(vec.to(torch.float32), val.to(torch.float32), [m.weight for m in chain],
                                     [m.bias for m in chain], seed)
        for fc in self.post_mlp:
            pe = fc(pe, act="relu")
        return pe

    def forward(self, batch):
        if getattr(batch, "eigvecs_sn", None) is None or getattr(batch, "eigvals_sn", None) is None:
            raise ValueError("Precomputed Laplacian statistics are required for LapPENodeEncoder; "
                             "transform.compute_posenc_stats_device(batch, is_undirected, cfg) attaches "
                             "batch.eigvecs_sn / batch.eigvals_sn")
        pe = self.pe(batch.eigvecs_sn, batch.eigvals_sn)
        h = self.linear_x(batch.x.to(torch.float32)) if self.expand_x else batch.x
        batch.x = torch.cat((h, pe), 1)
        if self.pass_as_var:
            batch.pe_LapPE = pe
        return batch
