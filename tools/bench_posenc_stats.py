#!/usr/bin/env python3
"""The Laplacian statistics of the positional encoding (graph_hscn/transform/posenc.py) three ways on the SAME seeded
graphs of ``loader.synthetic.make_dataset``: the host path (``compute_posenc_stats``, numpy ``eigh`` per graph), the
batched rocSOLVER path (``compute_posenc_stats_batched``) and the one-launch Jacobi kernel
(``compute_posenc_stats_device``, csrc/lap_eig.hip), "sym" Laplacian, L2 vectors, 10 frequencies.  Sets: 1024
Peptides-shaped graphs in batches of 128, 2048 PCQM-Contact-shaped in batches of 256, 128 PascalVOC-SP-shaped in
batches of 32.  Read-only towards the package.

Timing: a host clock around one pass over the set that ends in a device synchronise, after a warm-up pass over the
first batch; ``--passes`` passes per number, the median reported with the spread (max - min) / median.  The host and
rocSOLVER paths are timed on the first ``--host-graphs`` / ``--batched-batches`` of the set (they are slow; the counts
are in the output).  ``device_launch`` is the kernel on batches already collated on the device (what
``compute_posenc(stats="device")`` pays), ``device_list`` the list form end to end (collate, copy in, launch, one copy
back), the drop-in for the batched path.  Also written: sweep counts, the LDS / global tier split, and for the
tier-boundary and n = 444 / 500 graphs of tests/test_gpu_lap_eig.py the error of the kernel and of the host float32
path against float64 with their ratio.  Writes profiles/r07_posenc_stats.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import numpy as np
import torch

from graph_hscn import _hip
from graph_hscn.config.config import PEConfig
from graph_hscn.data import Batch, Data
from graph_hscn.loader.synthetic import SHAPES, make_dataset, make_graph
from graph_hscn.transform.posenc import (_dense_laplacian, compute_posenc_stats, compute_posenc_stats_batched,
                                         compute_posenc_stats_device)

DEV = "cuda"
CFG = PEConfig(9, 16, 8, eigen_max_freqs=10, eigen_laplacian_norm="sym", eigvec_norm="L2")


def _bare(graphs):
    """Fresh containers without statistics (and without features: the sets differ in width, the statistics do not
    read them)."""
    return [Data(x=torch.zeros(g.num_nodes, 1), edge_index=g.edge_index, num_nodes=g.num_nodes) for g in graphs]


def timed(fn, count, passes, warm):
    warm()
    torch.cuda.synchronize()
    s = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    med = statistics.median(s)
    return {"graphs": count, "seconds": med, "graphs_per_s": count / med, "spread": (max(s) - min(s)) / med,
            "passes": passes}


def case(name, count, bs, a):
    graphs = make_dataset(name, count, seed=0)
    chunks = [graphs[i:i + bs] for i in range(0, count, bs)]
    lds_max = _hip.lib().hscn_lap_eig_lds_max_n()
    ns = [g.num_nodes for g in graphs]
    row = {"graphs": count, "batch": bs, "nodes_mean": float(np.mean(ns)), "nodes_max": int(max(ns)),
           "lds_tier_graphs": int(sum(n <= lds_max for n in ns)), "global_tier_graphs": int(sum(n > lds_max for n in ns))}
    hg = _bare(graphs[:a.host_graphs])
    row["host"] = timed(lambda: [compute_posenc_stats(g, True, CFG) for g in hg], len(hg), 1,
                        lambda: [compute_posenc_stats(g, True, CFG) for g in _bare(graphs[:4])])
    bc = chunks[:a.batched_batches]
    row["batched_rocsolver"] = timed(lambda: [compute_posenc_stats_batched(_bare(c), True, CFG, device=DEV) for c in bc],
                                     sum(len(c) for c in bc), a.passes,
                                     lambda: compute_posenc_stats_batched(_bare(chunks[0]), True, CFG, device=DEV))
    row["device_list"] = timed(lambda: [compute_posenc_stats_device(_bare(c), True, CFG, device=DEV) for c in chunks],
                               count, a.passes, lambda: compute_posenc_stats_device(_bare(chunks[0]), True, CFG, device=DEV))
    dev = [Batch.from_data_list(c).to(DEV) for c in chunks]
    row["device_launch"] = timed(lambda: [compute_posenc_stats_device(b, True, CFG) for b in dev], count, a.passes,
                                 lambda: compute_posenc_stats_device(dev[0], True, CFG))
    sw = torch.cat([b.lap_eig_sweeps for b in dev]).cpu().numpy()
    row["flag"] = int(max(int(b.lap_eig_flag.item()) for b in dev))
    row["sweeps"] = {"min": int(sw.min()), "median": float(np.median(sw)), "max": int(sw.max())}
    row["launch_over_host"] = row["device_launch"]["graphs_per_s"] / row["host"]["graphs_per_s"]
    row["launch_over_batched"] = row["device_launch"]["graphs_per_s"] / row["batched_rocsolver"]["graphs_per_s"]
    row["list_over_batched"] = row["device_list"]["graphs_per_s"] / row["batched_rocsolver"]["graphs_per_s"]
    return row


def error_ratios():
    """Kernel and host float32 path against float64 eigh of the same float32 matrix (lower triangle mirrored), first
    10 eigenvalues clamped at 0 and the eigen-equation residual of the L2-normalised vectors."""
    m = _hip.lib().hscn_lap_eig_lds_max_n()
    rng7, rng11 = np.random.default_rng(7), np.random.default_rng(11)
    graphs = {f"lds_edge_n{m}": make_graph(rng7, SHAPES["peptides_func"], n=m),
              f"global_edge_n{m + 1}": make_graph(rng7, SHAPES["peptides_func"], n=m + 1),
              "n444": make_graph(rng11, SHAPES["peptides_func"], n=444),
              "n500": make_graph(rng11, SHAPES["pascalvoc_sp"], n=500)}
    out = {}
    for lap in ("sym", "none"):
        cfg = PEConfig(9, 16, 8, eigen_max_freqs=10, eigen_laplacian_norm=lap)
        dev = compute_posenc_stats_device(_bare(graphs.values()), True, cfg, device=DEV)
        for (name, g), d in zip(graphs.items(), dev):
            L = _dense_laplacian(g.edge_index.numpy(), g.num_nodes, None if lap == "none" else lap).astype(np.float64)
            L = np.tril(L) + np.tril(L, -1).T
            lam = np.linalg.eigvalsh(L)[:10]
            h = compute_posenc_stats(_bare([g])[0], True, cfg)
            r = {}
            for tag, s in (("device", d), ("host", h)):
                V = s.eigvecs_sn.numpy().astype(np.float64)
                V = V / np.linalg.norm(V, axis=0, keepdims=True)
                r[f"eig_err_{tag}"] = float(np.abs(s.eigvals_sn[0, :, 0].numpy() - np.maximum(lam, 0)).max())
                r[f"residual_{tag}"] = float(np.abs(L @ V - V * lam[None]).max())
            r["eig_ratio"] = r["eig_err_device"] / max(r["eig_err_host"], 1e-30)
            r["residual_ratio"] = r["residual_device"] / max(r["residual_host"], 1e-30)
            out[f"{name}_{lap}"] = r
    out["worst_eig_ratio"] = max(v["eig_ratio"] for v in out.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_posenc_stats.json"))
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-graphs", type=int, default=128)
    ap.add_argument("--batched-batches", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posenc_stats.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "lap_norm": "sym", "eigvec_norm": "L2", "max_freqs": 10,
           "lds_max_n": _hip.lib().hscn_lap_eig_lds_max_n()}
    for key, (name, count, bs) in {"peptides_func_1024_b128": ("peptides_func", 1024, 128),
                                   "pcqm_contact_2048_b256": ("pcqm_contact", 2048, 256),
                                   "pascalvoc_sp_128_b32": ("pascalvoc_sp", 128, 32)}.items():
        res[key] = case(name, count, bs, a)
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    res["error_ratios"] = error_ratios()
    print(json.dumps(res["error_ratios"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
