#!/usr/bin/env python3
"""The link-level head, measured: three things on the candidate pairs of a "pcqm_contact_link" batch of 256 graphs.

  pair_dot    forward + backward of ``nn.head.pair_dot`` (hscn_pair_dot_fwd / _bwd; the pair structure is built once,
              outside the timed region, as a training step does per batch) against the same computation in plain torch
              device ops: ``(z.index_select(0, u) * z.index_select(0, v)).sum(1)`` and autograd's index_add backward.
              Embedding widths D = 16 and D = 64; the embeddings are random, they only give the head something to chew.
  pair_rank   ``metrics.pair_rank_launch`` (hscn_pair_rank + hscn_pair_rank_reduce, filter 1) against
              ``metrics.link_rank_counts`` run on the device with torch ops (a per-graph Python loop: the restatement,
              not a contender).
  step        one whole link-level HSCN training step through the eager loop's calls: forward, BCE criterion,
              backward, Adam step (H = 16, D = 16, 4 clusters, 2 layers).

There is no ratio to meet: the HIP kernels are the only route of the library.  The numbers inform.  Read-only towards
the package.

Timing: HIP events around ``reps`` calls (the restatement and the step: a host clock around calls that end in a
synchronise); one untimed region per side as the warm-up, then ``regions`` such regions per number, the two sides of a
comparison alternating, the median reported with the spread (max - min) / median.  Writes
profiles/link_head_bench.json (--out)."""
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

from graph_hscn import metrics
from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import Batch, HeteroBatch
from graph_hscn.loader.hetero_data import hetero_from_clusters
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.hscn import HSCN
from graph_hscn.nn.head import PairStructure, pair_dot

DEV = "cuda"


def region(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_region(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def summary(us):
    med = statistics.median(us)
    return {"us": med, "spread": (max(us) - min(us)) / med}


def alternate(sides, regions, reps, timer=region):
    count = lambda k: reps[k] if isinstance(reps, dict) else reps
    for k, fn in sides.items():                   # warm-up: one untimed region of the same length per side
        timer(fn, count(k))
    us = {k: [] for k in sides}
    for _ in range(regions):                      # alternating: both sides see the same neighbours on the machine
        for k, fn in sides.items():
            us[k].append(timer(fn, count(k)))
    return {k: summary(v) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_head_bench.json"))
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_link_head.py measures on the HIP device: none found")
    graphs = make_dataset("pcqm_contact_link", a.graphs, seed=0)
    batch = Batch.from_data_list(graphs).to(DEV)
    N, P = int(batch.num_nodes), int(batch.edge_label_index.size(1))
    u, v = batch.edge_label_index
    structure = PairStructure.of(batch)
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "N": N, "P": P, "reps": a.reps,
           "regions": a.regions, "pair_dot": {}, "pair_rank": {}}
    gen = torch.Generator().manual_seed(0)
    for D in (16, 64):
        z = torch.randn(N, D, generator=gen).to(DEV).requires_grad_(True)
        g = (torch.randn(P, generator=gen) / P).to(DEV)

        def hip():
            return torch.autograd.grad(pair_dot(z, batch.edge_label_index, structure), z, g)

        def eager():
            return torch.autograd.grad((z.index_select(0, u) * z.index_select(0, v)).sum(1), z, g)

        out = alternate({"hip": hip, "torch": eager}, a.regions, a.reps)
        out["max_abs_difference"] = float((hip()[0] - eager()[0]).abs().max())
        res["pair_dot"][f"D{D}"] = out

        zd = z.detach()

        def rank_hip():
            return metrics.pair_rank_launch(zd, batch.ptr32, batch.pair_ptr32, structure, 1, want_rank2=False,
                                            max_nodes=int(batch.max_nodes))

        def rank_torch():
            return metrics.link_rank_counts(zd, batch.ptr, batch.pair_ptr32, batch.edge_label_index, batch.edge_label, 1)

        out = alternate({"hip": rank_hip, "torch": rank_torch}, a.regions, {"hip": a.reps, "torch": 1}, host_region)
        res["pair_rank"][f"D{D}"] = out

    # one whole link-level training step
    rng = np.random.default_rng(0)
    hb = HeteroBatch.from_data_list([hetero_from_clusters(g_, rng.integers(0, 4, g_.num_nodes), 4, "link")
                                     for g_ in graphs]).to(DEV)
    torch.manual_seed(0)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 16, 2, task_level="link").to(DEV)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        optimizer.zero_grad()
        loss, _ = criterion("cross_entropy", model(hb.x_dict, hb.edge_index_dict, hb), hb["local"].edge_label)
        loss.backward()
        optimizer.step()

    res["step"] = alternate({"hscn_link": step}, a.regions, max(a.reps // 5, 1), host_region)["hscn_link"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
