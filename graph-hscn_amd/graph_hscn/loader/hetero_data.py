"""Cluster assignments -> heterogeneous (local / virtual) graphs.

Same entry points and result layout as the reference
(/root/reference/graph_hscn/loader/hetero_data.py:14-106), quirks kept
(SURVEY.md Appendix B.1): virtual node v carries the float64 mean features of
remapped cluster (v+1) mod U (:52-59), vv edges are {(i -> j): i + j <= U-1}
(:68-79), lv edges point node ix at ``clusters[ix]`` (:80-86).

The reference's per-node Python loop with ``.tolist()`` round trips is replaced
by one vectorised pass per graph (host integer bookkeeping, as in the
reference, which also runs this stage on the host); results are bit-identical
(tests/test_host_logic.py); `hetero_batch_on_device` does the transform and the collate on the GPU (tests/test_gpu_hetero_device.py).
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from ..data import Data, DataLoader, HeteroData, has_link_labels

LL = ("local", "to", "local")
VV = ("virtual", "to", "virtual")
LV = ("local", "to", "virtual")


def hetero_from_clusters(data: Data, clusters_raw: Sequence[int], num_clusters: int,
                         task_level: str = "graph") -> HeteroData:
    """One graph of the loop body hetero_data.py:42-87.  ``task_level="link"``: the graph's candidate pairs and their
    labels (``edge_label_index`` / ``edge_label``, local node ids) travel on the local node type."""
    clusters_raw = np.asarray(clusters_raw).reshape(-1)
    n = int(data.num_nodes)
    if clusters_raw.shape[0] != n:
        raise ValueError("one cluster id per node expected")
    uniq, inv = np.unique(clusters_raw, return_inverse=True)        # :46-51 remap to 0..U-1
    U = int(uniq.shape[0])
    if U > num_clusters:
        raise IndexError("more distinct cluster ids than num_clusters")  # list index error at :54
    x64 = data.x.detach().cpu().numpy().astype(np.float64)
    sums = np.zeros((U, x64.shape[1]), dtype=np.float64)
    np.add.at(sums, inv, x64)                                        # node order, like np.mean over the lists
    cnt = np.bincount(inv, minlength=U).astype(np.float64)
    mean = sums / cnt[:, None]
    # slot index clusters[ix]-1 (:53): cluster 0 lands last => virtual v <- cluster (v+1) mod U
    virt = mean[(np.arange(U) + 1) % U].astype(np.float32)

    lens = U - np.arange(U)
    vv_src = np.repeat(np.arange(U), lens)                           # :68-70  [i]*(U-i)
    vv_dst = np.concatenate([np.arange(m) for m in lens]) if U else np.zeros(0, dtype=np.int64)  # :71-76

    h = HeteroData()
    h["local"].x = data.x.float()                                    # :64
    h["local"].y = data.y                                            # :65
    h["virtual"].x = torch.from_numpy(virt)                          # :66
    h[LL].edge_index = data.edge_index                               # :67
    h[VV].edge_index = torch.from_numpy(np.stack([vv_src, vv_dst]).astype(np.int64))      # :77-79
    h[LV].edge_index = torch.from_numpy(np.stack([np.arange(n), inv]).astype(np.int64))   # :80-86
    h["local"].num_nodes = n
    h["virtual"].num_nodes = U
    if task_level == "link":
        if not has_link_labels(data):
            raise ValueError("task_level='link' needs graphs with edge_label_index / edge_label")
        h["local"].edge_label_index = data.edge_label_index
        h["local"].edge_label = data.edge_label
    return h


def _check_task_level(data_cfg) -> None:
    level = getattr(data_cfg, "task_level", "graph")
    if level not in ("graph", "node", "link"):
        raise NotImplementedError(f"task_level {level!r} (graph- and node-level tasks are served)")


def generate_hetero_data(cluster_lst: list, dataset, split_idx: Dict[str, torch.Tensor], data_cfg, model_cfg,
                         logger=None) -> List[HeteroData]:
    """hetero_data.py:14-88: graphs come back ordered train || val || test.  ``task_level="node"`` (extension: the
    reference raises NotImplementedError for it) is the same per-graph transform; ``y`` is then one label per local
    node and travels on the local node type as it is.  ``task_level="link"`` copies the candidate pairs and their
    labels onto the local node type (``hetero_from_clusters``)."""
    _check_task_level(data_cfg)
    out: List[HeteroData] = []
    for split_name in ("train", "val", "test"):
        if logger is not None:
            logger.info(f"Generating heterogeneous dataset with virtual nodes for {split_name} split...")
        for i in split_idx[split_name]:
            i = int(i)
            out.append(hetero_from_clusters(dataset[i], cluster_lst[i], model_cfg.num_clusters,
                                            getattr(data_cfg, "task_level", "graph")))
    return out


def hetero_loaders(data_cfg, hetero_dataset: List[HeteroData], split_idx: Dict[str, torch.Tensor]) -> list:
    """hetero_data.py:91-106, including its re-indexing of the split-ordered list by
    the original dataset indices (quirk B.1-8).  ``task_level="node"`` is served like "graph": the collate
    concatenates the per-node labels."""
    _check_task_level(data_cfg)
    parts = [[hetero_dataset[int(i)] for i in split_idx[k]] for k in ("train", "val", "test")]
    return [
        DataLoader(parts[0], data_cfg.batch_size, shuffle=True, num_workers=data_cfg.num_workers),
        DataLoader(parts[1], data_cfg.batch_size, shuffle=False, num_workers=data_cfg.num_workers),
        DataLoader(parts[2], data_cfg.batch_size, shuffle=False, num_workers=data_cfg.num_workers),
    ]


def hetero_batch_on_device(batch, clusters: torch.Tensor, num_clusters: int):
    """Transform + collate in one step ON THE DEVICE: a block-diagonal ``Batch`` of raw graphs (on
    'cuda') and the raw cluster id of every node (int64 ``[N]``, e.g. the argmax of stage A, still on
    the device) -> the ``HeteroBatch`` the reference would obtain by running
    ``generate_hetero_data`` per graph (hetero_data.py:42-87) and collating.  Bit-identical to the host
    path (``hetero_from_clusters`` + ``HeteroBatch.from_data_list``); one host read of the two
    totals (V, E_vv) sizes the outputs."""
    from .. import _hip
    from ..data import HeteroBatch
    dev = batch.x.device
    if dev.type != "cuda":
        raise RuntimeError("hetero_batch_on_device works on device-resident batches")
    K = int(num_clusters)
    N, F = batch.x.shape
    B = int(batch.num_graphs)
    x = batch.x.contiguous()
    if x.dtype not in (torch.int64, torch.float32):
        x = x.float()
    nptr = batch.ptr32 if ("ptr32" in batch and batch.ptr32.device == dev) else batch.ptr.to(dev).to(torch.int32)
    clusters = clusters.to(torch.int64).contiguous()
    U = torch.empty(B, dtype=torch.int32, device=dev)
    lvl = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    means = torch.empty(B, K, F, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _hip.call("hscn_build_hetero_count", _hip.ptr(x), int(x.dtype == torch.int64), _hip.ptr(clusters), _hip.ptr(nptr),
              B, F, K, _hip.ptr(U), _hip.ptr(lvl), _hip.ptr(means), _hip.ptr(flag), _hip.stream())
    vptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    evptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    vptr32 = torch.empty(B + 1, dtype=torch.int32, device=dev)
    evptr32 = torch.empty(B + 1, dtype=torch.int32, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    _hip.call("hscn_build_hetero_scan", _hip.ptr(U), B, _hip.ptr(flag), _hip.ptr(vptr), _hip.ptr(evptr),
              _hip.ptr(vptr32), _hip.ptr(evptr32), _hip.ptr(totals), _hip.stream())
    V, Evv, bad, maxU = (int(t) for t in totals.cpu())                                       # the one host read
    if bad:
        raise IndexError("cluster ids must lie in [0, num_clusters)")
    vx = torch.empty(V, F, dtype=torch.float32, device=dev)
    ei_lv = torch.empty(2, N, dtype=torch.int64, device=dev)
    ei_vv = torch.empty(2, Evv, dtype=torch.int64, device=dev)
    vbatch = torch.empty(V, dtype=torch.int64, device=dev)
    _hip.call("hscn_build_hetero_emit", _hip.ptr(U), _hip.ptr(vptr), _hip.ptr(evptr), _hip.ptr(nptr), _hip.ptr(lvl),
              _hip.ptr(means), B, F, K, N, Evv, _hip.ptr(vx), _hip.ptr(ei_lv), _hip.ptr(ei_vv), _hip.ptr(vbatch),
              _hip.stream())
    hb = HeteroBatch()
    hb.num_graphs = B
    loc, vir = hb["local"], hb["virtual"]
    loc.x = batch.x.float()
    if "y" in batch and batch.y is not None:
        loc.y = batch.y
    loc.batch = batch.batch if batch.batch.device == dev else batch.batch.to(dev)
    loc.ptr = batch.ptr if batch.ptr.device == dev else batch.ptr.to(dev)
    loc.ptr32 = nptr
    loc.max_nodes = int(batch.max_nodes) if "max_nodes" in batch else int((loc.ptr[1:] - loc.ptr[:-1]).max())
    loc.num_nodes = N
    vir.x = vx
    vir.ptr = vptr
    vir.ptr32 = vptr32
    vir.batch = vbatch
    vir.max_nodes = maxU
    vir.num_nodes = V
    hb[LL].edge_index = batch.edge_index
    hb[LL].ptr32 = batch.eptr32 if batch.eptr32.device == dev else batch.eptr32.to(dev)
    hb[LL].max_edges = int(batch.max_edges)
    hb[VV].edge_index = ei_vv
    hb[VV].ptr32 = evptr32
    hb[VV].max_edges = maxU * (maxU + 1) // 2
    hb[LV].edge_index = ei_lv
    hb[LV].ptr32 = nptr
    hb[LV].max_edges = loc.max_nodes
    return hb
