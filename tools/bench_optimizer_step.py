#!/usr/bin/env python3
"""The stepping iteration of ``fit_resident`` with each optimizer path, on the Peptides-func batch (B = 128, H = 16,
L = 3): gather + one-launch step + gradient fold + optimizer update, timed with device events around runs of
iterations.  Four cases, built the way ``train_resident`` builds them:

  adamw_constant     AdamW at a constant rate -- ``optim.FlatAdam``, the whole iteration one graph replay
  adamw_cosine       the same with ``scheduler="cosine_with_warmup"`` evaluated inside the launch
  adagrad_flat       ``optim.FlatAdagrad``: one launch, inside the graph
  adagrad_eager      torch's Adagrad (``flat_optimizer=False``): the step graph, then the eager multi-launch update

Every case steps on every iteration (k = 1, no clip).  The cases alternate inside each of the 7 regions; per case the
median over the regions and the spread (min, max) are reported, and the JSON goes to profiles/r10_optimizer_step.json."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import numpy as np
import torch

from graph_hscn.config.config import ACT_DICT, OptimConfig
from graph_hscn.loader.device_dataset import DeviceHeteroDataset
from graph_hscn.loader.hetero_data import hetero_from_clusters
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.hscn import HSCN
from graph_hscn.replay import CapturedStep
from graph_hscn.train import train_resident as TR

CASES = {
    "adamw_constant": (OptimConfig("adamW", lr=1e-3), True),
    "adamw_cosine": (OptimConfig("adamW", lr=1e-3, scheduler="cosine_with_warmup", warmup_epochs=1), True),
    "adagrad_flat": (OptimConfig("adagrad", lr=1e-2), True),
    "adagrad_eager": (OptimConfig("adagrad", lr=1e-2), False),
}


def build_case(cfg, flat_optimizer, hs, dev, B, epochs):
    """The objects ``fit_resident`` builds for this configuration: ``iteration()`` is one stepping iteration."""
    torch.manual_seed(0)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(dev)
    model.engine = "resident"
    model.train()
    ds = DeviceHeteroDataset(hs, dev, B)
    gen = torch.Generator(device=dev).manual_seed(0)
    ds.new_epoch(gen)
    flat = flat_optimizer and cfg.optim_type in TR.FLAT_OPTIMIZERS
    num_batches = len(hs) // B
    schedule = TR.schedule_from_config(cfg, epochs, num_batches, 1)
    optimizer, in_graph = TR._make_optimizer(cfg, model, flat, False, False, schedule)
    step = CapturedStep(model, ds.static, "cross_entropy", optimizer=optimizer if in_graph else None,
                        pre=ds.gather_next)
    run = SimpleNamespace(step=step, optimizer=step.optimizer if flat else optimizer, reducer=None, flat=flat,
                          in_graph=in_graph, acc=False, clip_norm=None, flat_grads=step.step.grads[:step.step.P])
    if not in_graph:
        step.bind_grads()

    def iteration():
        step.replay()
        if not in_graph:
            TR._boundary_outside_graph(run, float(B))

    def new_epoch():
        ds.new_epoch(gen)

    return SimpleNamespace(iteration=iteration, new_epoch=new_epoch, in_graph=in_graph, ds=ds,
                           optimizer=type(run.optimizer).__name__, steps=num_batches)


def main(G, B, K, regions, epochs_per_region, out_path):
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer_step needs the MI355X: no HIP device")
    dev = torch.device("cuda:0")
    graphs = make_dataset("peptides_func", G, seed=0)
    rng = np.random.default_rng(0)
    hs = [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]
    total_epochs = (regions + 1) * epochs_per_region
    cases = {name: build_case(cfg, flat, hs, dev, B, total_epochs) for name, (cfg, flat) in CASES.items()}
    times = {name: [] for name in cases}

    def region(c):
        """``epochs_per_region`` epochs of stepping iterations between two device events: microseconds each."""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(epochs_per_region):
            c.new_epoch()
            for _ in range(c.steps):
                c.iteration()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / (epochs_per_region * c.steps)

    for c in cases.values():               # warm-up: every graph and every eager launch of the timed window
        region(c)
    for _ in range(regions):
        for name, c in cases.items():      # alternating: a drift of the machine reaches every case alike
            times[name].append(region(c))
    out = {"graphs": G, "graphs_per_batch": B, "hidden": 16, "layers": 3, "regions": regions,
           "iterations_per_region": epochs_per_region * (G // B), "unit": "us per stepping iteration", "cases": {}}
    for name, c in cases.items():
        c.ds.check()
        t = times[name]
        out["cases"][name] = {"optimizer": c.optimizer, "in_graph": c.in_graph, "median_us": statistics.median(t),
                              "min_us": min(t), "max_us": max(t), "regions_us": t}
    m = {n: out["cases"][n] for n in cases}
    spread = max(m["adamw_constant"]["max_us"] - m["adamw_constant"]["min_us"],
                 m["adamw_cosine"]["max_us"] - m["adamw_cosine"]["min_us"])
    out["scheduled_minus_constant_us"] = m["adamw_cosine"]["median_us"] - m["adamw_constant"]["median_us"]
    out["spread_of_the_two_us"] = spread
    out["scheduled_within_spread"] = out["scheduled_minus_constant_us"] <= spread
    out["adagrad_eager_over_flat"] = m["adagrad_eager"]["median_us"] / m["adagrad_flat"]["median_us"]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=16)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--epochs-per-region", type=int, default=200, help="epochs of graphs // batch iterations per region")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_optimizer_step.json"))
    a = ap.parse_args()
    main(a.graphs, a.batch, a.clusters, a.regions, a.epochs_per_region, a.out)
