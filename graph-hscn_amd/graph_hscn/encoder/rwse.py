"""Node encoder of the random-walk structural encoding (transform/rwse.py): the ``ksteps`` return probabilities of a
node, optionally batch-normalised, go through one Linear ("linear") or a stack of Linear + ReLU ("mlp") to ``dim_pe``
columns, which are appended to the (optionally expanded) node features -- the kernel-PE node encoder of the LRGB
baselines, built from the library's own modules: every flop is a HIP kernel (csrc/linear.hip with the ReLU in its
epilogue, csrc/norm.hip) and autograd runs through ``LinearFn`` / ``BatchNormFn``."""
from __future__ import annotations

import torch
import torch.nn as nn

from ..nn import BatchNorm1d, Linear


class RWSENodeEncoder(nn.Module):
    def __init__(self, cfg, dim_in: int, dim_emb: int, expand_x: bool = True) -> None:
        super().__init__()
        dim_pe, K = int(cfg.dim_pe), int(cfg.ksteps)
        if cfg.model not in ("linear", "mlp"):
            raise ValueError(f"Unexpected RWSE model {cfg.model}")
        if cfg.layers < 1:
            raise ValueError("Num layers in the RWSE encoder has to be positive.")
        if dim_emb - dim_pe < 1:
            raise ValueError(f"RWSE size {dim_pe} is too large for desired embedding size of {dim_emb}.")
        self.model_type = cfg.model
        self.pass_as_var = cfg.pass_as_var
        self.expand_x = expand_x
        if expand_x:
            self.linear_x = Linear(dim_in, dim_emb - dim_pe)
        self.raw_norm = BatchNorm1d(K) if cfg.raw_norm == "batchnorm" else None
        if cfg.model == "linear":
            widths = [K, dim_pe]
        elif cfg.layers == 1:
            widths = [K, dim_pe]
        else:
            widths = [K] + [2 * dim_pe] * (cfg.layers - 1) + [dim_pe]
        self.pe_encoder = nn.ModuleList(Linear(i, o) for i, o in zip(widths[:-1], widths[1:]))
        self._act = "identity" if cfg.model == "linear" else "relu"       # the linear kernel's epilogue

    def pe(self, rwse):
        """[N, dim_pe] from the random-walk statistics ``rwse`` [N, ksteps]."""
        pe = rwse.to(torch.float32)
        if self.raw_norm is not None:
            pe = self.raw_norm(pe)
        for fc in self.pe_encoder:
            pe = fc(pe, act=self._act)
        return pe

    def forward(self, batch):
        if getattr(batch, "rwse", None) is None:
            raise ValueError("Precomputed random-walk statistics are required for RWSENodeEncoder; "
                             "transform.compute_rwse_stats_device(batch, is_undirected, cfg) attaches batch.rwse")
        pe = self.pe(batch.rwse)
        h =self.linear_x(batch.x.to(torch.float32)) if self.expand_x else batch.x
        batch.x = torch.cat((h, pe), 1)
        if self.pass_as_var:
            batch.pe_rwse = pe
        return batch
