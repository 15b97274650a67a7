#!/usr/bin/env python3
"""HSCN with the ("virtual", "to", "local") relation (HSCN(vl_conv="GAT")) on a Peptides-func-shaped batch, H = 16,
K = 16, L = 3: the one-launch step (step.VLResidentTrainStep) replayed from a graph, the same model's layered autograd
step issued eagerly, and -- for context -- ResidentTrainStep on the three-relation model with the same batch, replayed
from a graph.  Read-only towards the package.

Timing (the method of tools/bench_gat_mpnn.py): HIP events around ``reps`` re-issues of one call, after a warm-up;
``regions`` such regions per number, the median reported with the spread (max - min) / median.
Writes profiles/r09_hscn_vl.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import numpy as np
import torch

from graph_hscn.config.config import ACT_DICT
from graph_hscn.data import HeteroBatch
from graph_hscn.loader.hetero_data import hetero_from_clusters
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.hscn import HSCN
from graph_hscn.step import ResidentTrainStep, VLResidentTrainStep

DEV = "cuda"


def timed(fn, reps, regions, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    med = statistics.median(us)
    return {"us": med, "spread": (max(us) - min(us)) / med}


def captured(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step.run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step.run()
    return g


def rows(B, K, reps, regions):
    rng = np.random.default_rng(0)
    graphs = make_dataset("peptides_func", B, seed=0)
    hb = HeteroBatch.from_data_list([hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]).to(DEV)
    out = {"graphs": B, "nodes": int(hb["local"].x.size(0)), "virtual_nodes": int(hb["virtual"].x.size(0)),
           "max_nodes": int(hb["local"].max_nodes)}
    torch.manual_seed(0)
    vl = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3, vl_conv="GAT").to(DEV)
    step = VLResidentTrainStep(vl, hb, "cross_entropy")
    g = captured(step)
    out["vl_one_launch_replayed"] = timed(g.replay, reps, regions)
    step.check()
    vl.engine = "layered"

    def layered():
        for p in vl.parameters():
            p.grad = None
        loss, _ = criterion("cross_entropy", vl(hb.x_dict, hb.edge_index_dict, hb), hb["local"].y)
        loss.backward()

    out["vl_layered_eager"] = timed(layered, max(reps // 10, 5), regions, warmup=5)
    torch.manual_seed(0)
    ref = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(DEV)
    rstep = ResidentTrainStep(ref, hb, "cross_entropy")
    g3 = captured(rstep)
    out["three_relation_resident_replayed"] = timed(g3.replay, reps, regions)
    rstep.check()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_hscn_vl.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hscn_vl.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "regions": a.regions, "H": 16, "K": 16, "L": 3,
           "batches": {}}
    for B in a.batches:
        res["batches"][str(B)] = rows(B, 16, a.reps, a.regions)
        print(f"B={B}", json.dumps(res["batches"][str(B)]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
