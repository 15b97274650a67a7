#!/usr/bin/env python3
"""The random-walk structural encoding (graph_hscn/transform/rwse.py, csrc/rwse.hip) on the seeded sets of
tools/bench_posenc_stats.py: 1024 Peptides-shaped graphs in batches of 128, 2048 PCQM-Contact-shaped in batches of 256,
128 PascalVOC-SP-shaped in batches of 32, ``ksteps = 20``.  Read-only towards the package.

Per set, in graphs/s:
* ``device_batch``: ``compute_rwse_stats_device`` on batches already collated on the device (what
  ``compute_posenc`` pays with an ``RWSEConfig``): the source-keyed CSR build plus the launch;
* ``csr_build`` and ``launch``: its two parts alone (``structure.build_csr``; ``hscn_rwse_stats`` over CSRs built
  beforehand);
* ``device_list``: the list form end to end (collate, copy in, CSR, launch, one copy back);
* ``lap_eig_device``: for comparison ``compute_posenc_stats_device`` ("sym", L2, 10 frequencies) on the same device
  batches -- a different computation (eigenpairs, not return probabilities); the table is what a user chooses by,
  there is no pass bar.

Timing: a host clock around one pass over the set that ends in a device synchronise, after a warm-up pass over the
first batch; ``--passes`` passes per number (default 3), the median reported with the spread (max - min) / median and
the window length in seconds (a short window measures launch overhead as much as the kernel: read ``seconds`` beside
the rate).  Writes profiles/rwse_bench.json (--out)."""
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
from graph_hscn.config.config import PEConfig, RWSEConfig
from graph_hscn.data import Batch, Data
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.structure import build_csr
from graph_hscn.transform import compute_posenc_stats_device, compute_rwse_stats_device

DEV = "cuda"
KSTEPS = 20
CFG = RWSEConfig(9, 16, 8, ksteps=KSTEPS)
LAP = PEConfig(9, 16, 8, eigen_max_freqs=10, eigen_laplacian_norm="sym", eigvec_norm="L2")


def _bare(graphs):
    """Fresh containers without statistics (and without features: the statistics do not read them)."""
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


def _csr(b):
    return build_csr(b.edge_index[0], b.edge_index[1], int(b.num_nodes), int(b.num_nodes))


def case(name, count, bs, a):
    graphs = make_dataset(name, count, seed=0)
    chunks = [graphs[i:i + bs] for i in range(0, count, bs)]
    ns = [g.num_nodes for g in graphs]
    T = _hip.lib().hscn_rwse_tile()
    row = {"graphs": count, "batch": bs, "nodes_mean": float(np.mean(ns)), "nodes_max": int(max(ns)),
           "edges_mean": float(np.mean([g.edge_index.size(1) for g in graphs])),
           "workgroups_per_batch": bs * ((max(ns) + T - 1) // T)}
    dev = [Batch.from_data_list(c).to(DEV) for c in chunks]
    row["device_batch"] = timed(lambda: [compute_rwse_stats_device(b, True, CFG) for b in dev], count, a.passes,
                                lambda: compute_rwse_stats_device(dev[0], True, CFG))
    row["flag"] = int(max(int(b.rwse_flag.item()) for b in dev))
    row["csr_build"] = timed(lambda: [_csr(b) for b in dev], count, a.passes, lambda: _csr(dev[0]))
    csrs = [_csr(b) for b in dev]
    outs = [(torch.empty(int(b.num_nodes), KSTEPS, dtype=torch.float32, device=DEV),
             torch.zeros(1, dtype=torch.int32, device=DEV)) for b in dev]

    def launches(items):
        for b, c, (rw, flag) in items:
            _hip.call("hscn_rwse_stats", _hip.ptr(c.rowptr), _hip.ptr(c.col), _hip.ptr(b.ptr32), int(b.num_nodes),
                      int(b.num_graphs), int(b.max_nodes), KSTEPS, _hip.ptr(rw), _hip.ptr(flag), _hip.stream())
    every = list(zip(dev, csrs, outs))
    row["launch"] = timed(lambda: launches(every), count, a.passes, lambda: launches(every[:1]))
    assert all(torch.equal(rw, b.rwse) for b, (rw, _) in zip(dev, outs)), "the two forms disagree"
    row["device_list"] = timed(lambda: [compute_rwse_stats_device(_bare(c), True, CFG, device=DEV) for c in chunks],
                               count, a.passes, lambda: compute_rwse_stats_device(_bare(chunks[0]), True, CFG, device=DEV))
    row["lap_eig_device"] = timed(lambda: [compute_posenc_stats_device(b, True, LAP) for b in dev], count, a.passes,
                                  lambda: compute_posenc_stats_device(dev[0], True, LAP))
    row["device_batch_over_lap_eig"] = row["device_batch"]["graphs_per_s"] / row["lap_eig_device"]["graphs_per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rwse_bench.json"))
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rwse.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "ksteps": KSTEPS, "tile": _hip.lib().hscn_rwse_tile(),
           "lap_eig": {"lap_norm": "sym", "eigvec_norm": "L2", "max_freqs": 10}}
    for key, (name, count, bs) in {"peptides_func_1024_b128": ("peptides_func", 1024, 128),
                                   "pcqm_contact_2048_b256": ("pcqm_contact", 2048, 256),
                                   "pascalvoc_sp_128_b32": ("pascalvoc_sp", 128, 32)}.items():
        res[key] = case(name, count, bs, a)
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
