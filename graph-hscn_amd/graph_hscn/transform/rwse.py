"""Random-walk structural encoding (RWSE): the return probabilities of the random walk after 1 .. K steps,
``rw[i, k-1] = (P^k)[i, i]`` with ``P = D^-1 A`` -- the positional statistics of the LRGB baselines that need no
eigensolver (no convergence test, no sign or rotation ambiguity, only non-negative sums).

Definition, the same on every path.  For one graph of ``n`` nodes with a directed edge list: ``A[r, c]`` is the number
of listed edges ``r -> c`` (duplicates sum; self loops are kept as listed, unlike the Laplacian path, which drops
them), ``deg[r] = sum_c A[r, c]`` the out-degree, ``P[r, c] = A[r, c] / deg[r]`` with an all-zero row where
``deg[r] = 0``; the result is float32 ``[n, K]`` and a node without out-edges gets zeros.  ``is_undirected=True``: the
list is used as given (the loaders list both directions); ``is_undirected=False``: it is first replaced by
``posenc._undirected(edge_index)`` (both directions, duplicates merged) -- in Python, before the launch, synchronising.

* ``compute_rwse_stats``: the host path, a dense float32 torch restatement of the definition;
* ``compute_rwse_stats_device``: ONE launch of the library's kernel (csrc/rwse.hip, include/hscn.h: hscn_rwse_stats)
  over the batch's source-keyed CSR."""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from .posenc import _undirected


def _num_nodes(data) -> int:
    return int(data.num_nodes) if hasattr(data, "num_nodes") else int(data.x.shape[0])


def compute_rwse_stats(data, is_undirected: bool, cfg):
    """Attaches ``rwse`` float32 [n, cfg.ksteps] to ``data`` (see the module docstring) and returns it."""
    n, K = _num_nodes(data), int(cfg.ksteps)
    ei = data.edge_index.cpu()
    if not is_undirected:
        ei = _undirected(ei)
    A = torch.zeros(n, n, dtype=torch.float32)
    A.index_put_((ei[0], ei[1]), torch.ones(ei.size(1), dtype=torch.float32), accumulate=True)
    deg = A.sum(1)
    dinv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    P = dinv.unsqueeze(1) * A
    M = torch.eye(n, dtype=torch.float32)
    cols = []
    for _ in range(K):
        M = P @ M
        cols.append(torch.diagonal(M).clone())
    data.rwse = torch.stack(cols, 1) if cols else torch.zeros(n, 0, dtype=torch.float32)
    return data


def _rwse_launch(batch, is_undirected: bool, cfg) -> Tuple[Tensor, Tensor]:
    """hscn_rwse_stats on a device ``Batch``: ``(rw [N, K] f32, flag [1] i32)``, both on the device, nothing read
    back."""
    from .. import _hip
    from ..structure import build_csr
    ei = batch.edge_index
    _hip.ptr(ei)                                   # a CPU tensor raises here: there is no CPU fallback
    for attr in ("ptr32", "max_nodes", "num_graphs"):
        if not hasattr(batch, attr):
            raise ValueError(f"the batch carries no {attr} (graph_hscn.data.Batch.from_data_list builds it)")
    lib = _hip.lib()
    dev = ei.device
    K, max_n = int(cfg.ksteps), int(batch.max_nodes)
    B, N = int(batch.num_graphs), int(batch.num_nodes)
    if not lib.hscn_rwse_supported(max(max_n, 1), K):
        raise RuntimeError(f"compute_rwse_stats_device: the largest graph has {max_n} nodes and ksteps is {K}; "
                           "the kernel takes graphs of at most 512 nodes and at most 64 steps")
    if not is_undirected:
        ei = _undirected(ei)                       # synchronises (torch.unique); graph blocks stay graph blocks
    csr = build_csr(ei[0], ei[1], N, N)            # stable, keyed by SOURCE: row r lists the targets of r
    ptr32 = batch.ptr32 if batch.ptr32.device == dev else batch.ptr32.to(dev)
    rw = torch.empty(N, K, dtype=torch.float32, device=dev)
    # an end outside [0, N) never enters the CSR (the build skips it and says so): the same bit as an end outside
    # the edge's own graph, which the launch finds
    flag = csr.flag.ne(0).to(torch.int32) * 2
    _hip.call("hscn_rwse_stats", _hip.ptr(csr.rowptr), _hip.ptr(csr.col), _hip.ptr(ptr32), N, B, max_n, K,
              _hip.ptr(rw), _hip.ptr(flag), _hip.stream())
    return rw, flag


def compute_rwse_stats_device(batch_or_graphs, is_undirected: bool, cfg, device="cuda"):
    """The same statistics through ONE launch of the library's kernel (see the module docstring).

    * A ``graph_hscn.data.Batch`` on the device gets ``rwse [N, K]`` (what ``RWSENodeEncoder.forward`` reads) and
      ``rwse_flag`` ([1] int32 on the device: bit 1 an edge outside its graph, bit 2 a graph beyond the batch's
      ``max_nodes``; bit 0 unused, as in ``lap_eig_flag``); nothing is read back.  Returns the batch.
    * A list of ``Data`` is collated, run on ``device`` with one launch and gets per-graph CPU ``rwse`` tensors from
      one copy; a nonzero flag raises ``RuntimeError`` naming the graph.  Returns the list.

    CPU tensors raise (there is no CPU fallback), and so do graphs beyond 512 nodes or ``ksteps`` beyond 64."""
    from ..data import Batch
    if isinstance(batch_or_graphs, Batch):
        batch = batch_or_graphs
        batch.rwse, batch.rwse_flag = _rwse_launch(batch, is_undirected, cfg)
        return batch
    graphs = list(batch_or_graphs)
    host = Batch.from_data_list(graphs)
    dev = Batch(edge_index=host.edge_index.to(device), num_nodes=host.num_nodes)
    dev.ptr32 = host.ptr32.to(device)
    dev.max_nodes, dev.num_graphs = host.max_nodes, host.num_graphs
    rw, flag = _rwse_launch(dev, is_undirected, cfg)
    rw = rw.cpu()
    f = int(flag.item())
    ptr = host.ptr.tolist()
    if f:
        for b, g in enumerate(graphs):
            n = ptr[b + 1] - ptr[b]
            if bool(((g.edge_index < 0) | (g.edge_index >= n)).any()):
                raise RuntimeError(f"compute_rwse_stats_device: graph {b} has an edge with an end outside its {n} nodes")
        raise RuntimeError(f"compute_rwse_stats_device: the launch reported flag {f}")
    for b, g in enumerate(graphs):
        g.rwse = rw[ptr[b]:ptr[b + 1]]
    return graphs
