#!/usr/bin/env python3
"""The per-node head of a node-level step -- head forward, weighted criterion, head backward -- on two routes, both
replayed from a graph: "fused" (hscn_node_head_fwd, hscn_class_weights + hscn_softmax_nll_fwd_ex, hscn_node_head_bwd
consuming the criterion's gradient unmultiplied) and "layered" (two hscn_linear_fwd, the same criterion, hscn_scale,
hscn_act_bwd, two backward-x hscn_linear_fwd and two hscn_linear_bwd_w with their folds).  Two shapes: N = 20 584,
H = 16, C = 10 (the nodes of a Peptides-shaped batch of 128) and the nodes of a PascalVOC-shaped batch of 128 with
C = 21.  The rows are random: they only give the head something to chew.  A measurement, not a gate.  Read-only
towards the package.

Timing (the method of tools/bench_multiclass_step.py): HIP events around ``reps`` replays, after a warm-up;
``regions`` such regions per number, alternating between the routes, the median reported with the spread
(max - min) / median.  ``fused_is_faster``: the fused median beats the layered one by more than the larger of the two
absolute spreads.  Writes profiles/r12_node_head.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.nn import Linear
from graph_hscn.nn.head import NodeHead

DEV = "cuda"
LAUNCHES = {"fused": {"head_fwd": 1, "criterion": 5, "head_bwd": 2},
            "layered": {"head_fwd": 2, "criterion": 5, "scale": 1, "act_bwd": 1, "bwd_x": 2, "bwd_w": 4}}


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


def step_of(route, x, y, H, C):
    torch.manual_seed(0)
    lin_1, lin_2 = Linear(H, H).to(DEV), Linear(H, C).to(DEV)
    head = NodeHead(lin_1, lin_2, "relu", route=route)
    params = [lin_1.weight, lin_1.bias, lin_2.weight, lin_2.bias]

    def run():
        loss, _ = criterion("weighted_cross_entropy", head(x), y)
        return torch.autograd.grad(loss, [x] + params)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_node_head.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_node_head.py measures on the HIP device: none found")
    pascal = sum(g.num_nodes for g in make_dataset("pascalvoc_sp_node", 128, seed=0))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "regions": a.regions, "launches": LAUNCHES,
           "shapes": {}}
    for name, N, H, C in (("peptides_b128", 20584, 16, 10), ("pascalvoc_b128", pascal, 16, 21)):
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(N, H, generator=gen).to(DEV).requires_grad_(True)
        y = torch.randint(0, C, (N,), generator=gen).to(DEV)
        graphs = {route: captured(step_of(route, x, y, H, C)) for route in ("fused", "layered")}
        for g in graphs.values():
            for _ in range(20):
                g.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in graphs}
        for _ in range(a.regions):                # alternating: both routes see the same neighbours on the machine
            for k, g in graphs.items():
                us[k].append(region(g.replay, a.reps))
        out = {"N": N, "H": H, "C": C}
        out.update({k: summary(v) for k, v in us.items()})
        noise = max(out[k]["us"] * out[k]["spread"] for k in graphs)
        out["difference_us"] = out["layered"]["us"] - out["fused"]["us"]
        out["fused_is_faster"] = out["difference_us"] > noise
        res["shapes"][name] = out
    res["fused_is_faster_at_both"] = all(s["fused_is_faster"] for s in res["shapes"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
