#!/usr/bin/env python3
"""The class-index training step (step.ResidentTrainStep with int64 [B] targets: forward launch,
hscn_softmax_nll_fwd, backward launch) against the BCE launch pair (one_launch=False) on the SAME Peptides-func-shaped
batch: B = 128, H = 16, K = 16, L = 3, C = 10, both replayed from a graph.  The class labels are random: they only
give the step something to chew.  The criterion launch alone, replayed, is reported as well.  A measurement, not a
gate.  Read-only towards the package.

Timing (the method of tools/bench_hscn_vl.py): HIP events around ``reps`` replays, after a warm-up; ``regions`` such
regions per number, alternating between the two steps, the median reported with the spread (max - min) / median.
Writes profiles/r11_multiclass_step.json (--out)."""
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
from graph_hscn.loss import launch_softmax_nll
from graph_hscn.model.hscn import HSCN
from graph_hscn.step import ResidentTrainStep

DEV = "cuda"


def region(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def summary(us):
    med = statistics.median(us)
    return {"us": med, "spread": (max(us) - min(us)) / med}


def captured(run):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_multiclass_step.json"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiclass_step.py measures on the HIP device: none found")
    B, K, H, L, C = a.batch, 16, 16, 3, 10
    rng = np.random.default_rng(0)
    graphs = make_dataset("peptides_func", B, seed=0)
    hb = HeteroBatch.from_data_list([hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]).to(DEV)
    y_bce = hb["local"].y.float().contiguous()
    y_cls = torch.from_numpy(rng.integers(0, C, B)).to(DEV)
    torch.manual_seed(0)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, H, C, L).to(DEV)
    cls = ResidentTrainStep(model, hb, "cross_entropy", target=y_cls)
    pair = ResidentTrainStep(model, hb, "cross_entropy", target=y_bce, one_launch=False)
    assert cls.class_index and not cls.one_launch and not pair.one_launch
    graphs_ = {"class_index_three_launches": captured(cls.run), "bce_launch_pair": captured(pair.run),
               "softmax_nll_launch_alone": captured(lambda: launch_softmax_nll(
                   cls.pred, cls.target, cls._loss1, cls.score, cls.g_pred, cls.class_flags, cls._nll_ws))}
    for g in graphs_.values():
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    us = {k: [] for k in graphs_}
    for _ in range(a.regions):                    # alternating: both steps see the same neighbours on the machine
        for k, g in graphs_.items():
            us[k].append(region(g.replay, a.reps))
    cls.check()
    pair.check()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "regions": a.regions, "graphs": B, "H": H, "K": K,
           "L": L, "C": C, "nodes": int(hb["local"].x.size(0)), "virtual_on_own_workgroups": bool(cls.defer)}
    res.update({k: summary(v) for k, v in us.items()})
    res["difference_us"] = res["class_index_three_launches"]["us"] - res["bce_launch_pair"]["us"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
