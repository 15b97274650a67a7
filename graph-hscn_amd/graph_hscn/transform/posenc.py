"""Laplacian eigen-decomposition statistics for the SignNet positional encoding
(/root/reference/graph_hscn/transform/posenc.py:14-107), same names and return conventions.

This is dataset PRE-PROCESSING in the reference (loader/loader.py:74-90: once per graph, on the host, numpy ``eigh``),
not part of the training step.  Two back ends for the decomposition:

* ``device=None`` (default): the reference's own path -- dense Laplacian with numpy, ``np.linalg.eigh`` on the host;
* ``device="cuda"``: the batched form -- the graphs' Laplacians are assembled on the GPU as one zero-padded
  ``[B, nmax, nmax]`` tensor (padding rows carry a diagonal entry above the graph's spectrum, so their eigenpairs sort behind every real
  one and cannot mix with them) and decomposed by ONE batched ``torch.linalg.eigh`` (rocSOLVER): SURVEY.md 8(f)4.

Eigenvectors are defined up to sign, and up to a rotation inside a repeated eigenvalue's eigenspace (molecules have
many): the two back ends agree on eigenvalues, on ``L v = lambda v`` and on the projector of every eigenspace, not on
the entries of ``v`` -- which is exactly the ambiguity SignNet (encoder/signnet.py) is built to be invariant to.

``compute_posenc_stats_device`` is the third back end: ONE launch of the library's own batched Jacobi eigensolver
(csrc/lap_eig.hip, include/hscn.h: hscn_lap_eig_stats) takes a collated batch's ``edge_index`` to the ``[N, max_freqs]``
tensors the encoder reads -- no dense Laplacian in HBM, no padding to the largest graph, no host loop, no rocSOLVER."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor


def _undirected(edge_index: Tensor) -> Tensor:
    """PyG ``to_undirected`` without edge attributes: both directions, duplicates merged."""
    ei = torch.cat([edge_index, edge_index.flip(0)], 1)
    return torch.unique(ei, dim=1)


def _dense_laplacian(edge_index: np.ndarray, N: int, normalization: Optional[str]) -> np.ndarray:
    """PyG ``get_laplacian`` densified (``to_scipy_sparse_matrix(...).toarray()``): self loops removed, unit weights,
    duplicate edges summed; None: D - A; "sym": I - D^-1/2 A D^-1/2; "rw": I - D^-1 A."""
    row, col = edge_index
    keep = row != col
    row, col = row[keep], col[keep]
    A = np.zeros((N, N), dtype=np.float32)
    np.add.at(A, (row, col), np.float32(1.0))
    deg = np.zeros(N, dtype=np.float32)
    np.add.at(deg, row, np.float32(1.0))
    if normalization is None:
        return (np.diag(deg) - A).astype(np.float32)
    if normalization == "sym":
        with np.errstate(divide="ignore"):
            dis = deg ** np.float32(-0.5)
        dis[np.isinf(dis)] = 0.0
        return (np.eye(N, dtype=np.float32) - dis[:, None] * A * dis[None, :]).astype(np.float32)
    if normalization == "rw":
        with np.errstate(divide="ignore"):
            di = np.float32(1.0) / deg
        di[np.isinf(di)] = 0.0
        return (np.eye(N, dtype=np.float32) - di[:, None] * A).astype(np.float32)
    raise ValueError(f"unknown Laplacian normalization {normalization!r}")


def compute_posenc_stats(data, is_undirected: bool, cfg):
    """posenc.py:14-48: attaches ``eigvals_sn`` [N, max_freqs, 1] and ``eigvecs_sn`` [N, max_freqs] to ``data``."""
    N = int(data.num_nodes) if hasattr(data, "num_nodes") else int(data.x.shape[0])
    norm_type = cfg.eigen_laplacian_norm.lower()
    if norm_type == "none":
        norm_type = None
    ei = data.edge_index if is_undirected else _undirected(data.edge_index)
    L = _dense_laplacian(ei.cpu().numpy(), N, norm_type)
    evals_sn, evects_sn = np.linalg.eigh(L)
    data.eigvals_sn, data.eigvecs_sn = get_lap_decomp_stats(evals=evals_sn, evects=evects_sn,
                                                            max_freqs=cfg.eigen_max_freqs, eigvec_norm=cfg.eigvec_norm)
    return data


def compute_posenc_stats_batched(graphs: Sequence, is_undirected: bool, cfg, device="cuda") -> List:
    """The same statistics for a list of graphs with ONE batched device ``eigh`` (see the module docstring)."""
    norm_type = cfg.eigen_laplacian_norm.lower()
    if norm_type == "none":
        norm_type = None
    ns = [int(g.num_nodes) if hasattr(g, "num_nodes") else int(g.x.shape[0]) for g in graphs]
    nmax = max(ns)
    dev = torch.device(device)
    Ls = torch.zeros(len(graphs), nmax, nmax, dtype=torch.float32)
    for b, (g, n) in enumerate(zip(graphs, ns)):
        ei = g.edge_index if is_undirected else _undirected(g.edge_index)
        L = torch.from_numpy(_dense_laplacian(ei.cpu().numpy(), n, norm_type))
        Ls[b, :n, :n] = L
        if n < nmax:
            # padding: eigenvector e_i with an eigenvalue just above the graph's own spectrum (Gershgorin bound of the
            # matrix eigh reads, whichever triangle), so the graph's n pairs come first and keep their f32 precision
            bound = float(max(L.abs().sum(0).max(), L.abs().sum(1).max())) + 1.0
            idx = torch.arange(n, nmax)
            Ls[b, idx, idx] = bound
    evals, evects = torch.linalg.eigh(Ls.to(dev))
    evals, evects = evals.cpu().numpy(), evects.cpu().numpy()
    for b, (g, n) in enumerate(zip(graphs, ns)):
        g.eigvals_sn, g.eigvecs_sn = get_lap_decomp_stats(evals=evals[b, :n], evects=evects[b, :n, :n],
                                                        max_freqs=cfg.eigen_max_freqs, eigvec_norm=cfg.eigvec_norm)
    return list(graphs)


_LAP_NORMS = {"none": 0, "sym": 1, "rw": 2}
_VEC_NORMS = {"L1": 0, "L2": 1, "abs-max": 2}


def _lap_eig_launch(batch, is_undirected: bool, cfg) -> Tuple[Tensor, Tensor, Tensor]:
    """hscn_lap_eig_stats on a device ``Batch``: ``(out [2, N, k] = eigvals | eigvecs, flag [1] i32, sweeps [B] i32)``,
    all on the device, nothing read back."""
    from .. import _hip
    ei = batch.edge_index
    _hip.ptr(ei)                                   # a CPU tensor raises here: there is no CPU fallback
    lap = cfg.eigen_laplacian_norm.lower()
    if lap not in _LAP_NORMS:
        raise ValueError(f"unknown Laplacian normalization {cfg.eigen_laplacian_norm!r}")
    if cfg.eigvec_norm not in _VEC_NORMS:
        raise ValueError(f"Unsupported normalization `{cfg.eigvec_norm}`")
    for attr in ("ptr32", "eptr32", "max_nodes", "num_graphs"):
        if not hasattr(batch, attr):
            raise ValueError(f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)")
    lib = _hip.lib()
    dev = ei.device
    k, max_n = int(cfg.eigen_max_freqs), int(batch.max_nodes)
    B, N = int(batch.num_graphs), int(batch.num_nodes)
    if not lib.hscn_lap_eig_supported(max(max_n, 1), k):
        raise RuntimeError(f"compute_posenc_stats_device: the largest graph has {max_n} nodes and eigen_max_freqs is {k}; "
                           "the kernel takes graphs of at most 512 nodes and at most 64 frequencies")
    ei = ei.contiguous()
    ptr32 = batch.ptr32 if batch.ptr32.device == dev else batch.ptr32.to(dev)
    eptr32 = batch.eptr32 if batch.eptr32.device == dev else batch.eptr32.to(dev)
    out = torch.empty(2, N, k, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.hscn_lap_eig_workspace_bytes(B, max_n))
    ws = torch.empty(need + 4 * B, dtype=torch.uint8, device=dev)      # the B words behind: sweep counts
    sweeps = ws[need:].view(torch.int32)
    sweeps.zero_()
    _hip.call("hscn_lap_eig_stats", _hip.ptr(ei), ei.size(1), _hip.ptr(ptr32), _hip.ptr(eptr32), N, B, max_n,
              _LAP_NORMS[lap], int(bool(is_undirected)), k, _VEC_NORMS[cfg.eigvec_norm], _hip.ptr(out[0]),
              _hip.ptr(out[1]), _hip.ptr(flag), _hip.ptr(ws), ws.numel(), _hip.stream())
    return out, flag, sweeps


def compute_posenc_stats_device(batch_or_graphs, is_undirected: bool, cfg, device="cuda"):
    """The same statistics through ONE launch of the library's batched Jacobi eigensolver (see the module docstring).

    * A ``graph_hscn.data.Batch`` on the device gets ``eigvecs_sn [N, k]`` and ``eigvals_sn [N, k, 1]`` as device
      tensors (what ``SignNetNodeEncoder.forward`` reads), ``lap_eig_flag`` ([1] int32 on the device: bit 0 a graph
      reached the sweep cap, bit 1 an edge outside its graph, bit 2 a graph beyond the batch's ``max_nodes``) and
      ``lap_eig_sweeps`` ([B] int32); nothing is read back.  Returns the batch.
    * A list of ``Data`` is collated, decomposed on ``device`` and gets per-graph CPU tensors from one copy, like
      ``compute_posenc_stats_batched``; a nonzero flag raises ``RuntimeError`` naming the graph.  Returns the list.

    CPU tensors raise (there is no CPU fallback), and so do graphs beyond 512 nodes or ``eigen_max_freqs`` beyond 64."""
    from ..data import Batch
    if isinstance(batch_or_graphs, Batch):
        batch = batch_or_graphs
        out, flag, sweeps = _lap_eig_launch(batch, is_undirected, cfg)
        batch.eigvals_sn, batch.eigvecs_sn = out[0].unsqueeze(2), out[1]
        batch.lap_eig_flag, batch.lap_eig_sweeps = flag, sweeps
        return batch
    graphs = list(batch_or_graphs)
    host = Batch.from_data_list(graphs)
    dev = Batch(edge_index=host.edge_index.to(device), num_nodes=host.num_nodes)
    dev.ptr32, dev.eptr32 = host.ptr32.to(device), host.eptr32.to(device)
    dev.max_nodes, dev.num_graphs = host.max_nodes, host.num_graphs
    out, flag, sweeps = _lap_eig_launch(dev, is_undirected, cfg)
    vals, vecs = out.cpu()
    f = int(flag.item())
    if f:
        ptr, sw = host.ptr.tolist(), sweeps.cpu()
        if f & 1:
            raise RuntimeError(f"compute_posenc_stats_device: graph {int(sw.argmax())} reached the sweep cap "
                               f"({int(sw.max())} sweeps) without converging")
        for b, g in enumerate(graphs):
            n = ptr[b + 1] - ptr[b]
            if bool(((g.edge_index < 0) | (g.edge_index >= n)).any()):
                raise RuntimeError(f"compute_posenc_stats_device: graph {b} has an edge with an end outside its {n} nodes")
        raise RuntimeError(f"compute_posenc_stats_device: the launch reported flag {f}")
    ptr = host.ptr.tolist()
    for b, g in enumerate(graphs):
        g.eigvals_sn, g.eigvecs_sn = vals[ptr[b]:ptr[b + 1]].unsqueeze(2), vecs[ptr[b]:ptr[b + 1]]
    return graphs


def get_lap_decomp_stats(evals, evects, max_freqs: int, eigvec_norm: str = "L2") -> Tuple[Tensor, Tensor]:
    """posenc.py:51-83: the ``max_freqs`` smallest eigenpairs, eigenvalues clamped at 0, eigenvectors normalised,
    both NaN-padded to ``max_freqs`` columns; eigenvalues repeated per node -> [N, max_freqs, 1]."""
    N = len(evals)
    idx = evals.argsort()[:max_freqs]
    evals, evects = evals[idx], np.real(evects[:, idx])
    evals = torch.from_numpy(np.real(evals)).clamp_min(0)
    evects = torch.from_numpy(np.ascontiguousarray(evects)).float()
    evects = eigvec_normalizer(evects, evals, normalization=eigvec_norm)
    if N < max_freqs:
        eig_vecs = F.pad(evects, (0, max_freqs - N), value=float("nan"))
        eig_vals = F.pad(evals, (0, max_freqs - N), value=float("nan")).unsqueeze(0)
    else:
        eig_vecs = evects
        eig_vals = evals.unsqueeze(0)
    eig_vals = eig_vals.repeat(N, 1).unsqueeze(2)
    return eig_vals, eig_vecs


def eigvec_normalizer(eig_vecs: Tensor, eig_vals: Tensor, normalization: str = "L2", eps: float = 1e-12) -> Tensor:
    """posenc.py:86-107."""
    if normalization == "L1":
        denom = eig_vecs.norm(p=1, dim=0, keepdim=True)
    elif normalization == "L2":
        denom = eig_vecs.norm(p=2, dim=0, keepdim=True)
    elif normalization == "abs-max":
        denom = torch.max(eig_vecs.abs(), dim=0, keepdim=True).values
    else:
        raise ValueError(f"Unsupported normalization `{normalization}`")
    denom = denom.clamp_min(eps).expand_as(eig_vecs)
    return eig_vecs / denom
