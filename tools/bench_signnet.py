#!/usr/bin/env python3
"""One pass of the SignNet node encoder (the positional-encoding stage, train.compute_posenc) over a
Peptides-func-shaped batch of 128 and a PCQM-Contact-shaped batch of 256: the layered engine (per-operator kernels)
beside the one-launch kernel (csrc/signnet.hip) on the SAME batch and weights, default PEConfig widths.  Read-only
towards the package.

Timing: HIP events around ``reps`` re-issues of one encoder call under no_grad, after a warm-up; ``regions`` such
regions per number, the median reported with the spread (max - min) / median.  Launch counts: device kernels of ONE
call in a torch.profiler kernel trace (null when the profiler is not available).  The eigenvector channels are random
numbers of the right shape: the work does not depend on their values.  Writes profiles/r06_signnet.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

from graph_hscn.config.config import PEConfig
from graph_hscn.data import Batch
from graph_hscn.encoder import SignNetNodeEncoder
from graph_hscn.loader.synthetic import make_dataset

DEV = "cuda"


def timed(fn, reps, regions, warmup=10):
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


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                 and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        plain = [n.replace("(anonymous namespace)::", "").replace("void ", "") for n in names]
        short = sorted({n.split("<")[0].split("(")[0][:48] for n in plain})
        return {"kernels": len(names), "distinct": short} if names else None
    except Exception as e:      # the measurement above stands without the trace
        return {"error": repr(e)}


def case(name, count, K, reps, regions):
    cfg = PEConfig(9, 16, 8, eigen_max_freqs=K)
    graphs = make_dataset(name, count, seed=0)
    g = torch.Generator().manual_seed(0)
    for d in graphs:
        d.eigvecs_sn = torch.randn(d.num_nodes, K, generator=g)
        d.eigvals_sn = torch.zeros(d.num_nodes, K, 1)
    b = Batch.from_data_list(graphs).to(DEV)
    x0 = b.x.float().contiguous()
    torch.manual_seed(0)
    enc = SignNetNodeEncoder(cfg, 9, 16).to(DEV)
    row = {"graphs": count, "nodes": int(b.num_nodes), "edges": int(b.edge_index.size(1)), "max_nodes": int(b.max_nodes),
           "max_edges": int(b.max_edges), "K": K, "hidden": cfg.phi_hidden_dim}
    outs = {}
    for engine in ("layered", "resident"):
        enc.engine = engine

        def fn():
            b.x = x0
            with torch.no_grad():
                return enc(b).x

        outs[engine] = fn().clone()
        assert enc.last_engine == engine
        row[engine] = timed(fn, reps, regions)
        row[engine]["launches"] = launches(fn)
    row["max_abs_difference"] = float((outs["layered"] - outs["resident"]).abs().max())
    row["speedup"] = row["layered"]["us"] / row["resident"]["us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_signnet.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_signnet.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "regions": a.regions,
           "peptides_func_b128": case("peptides_func", 128, 10, a.reps, a.regions)}
    print(json.dumps(res["peptides_func_b128"]), file=sys.stderr, flush=True)
    res["pcqm_contact_b256"] = case("pcqm_contact", 256, 10, a.reps, a.regions)
    print(json.dumps(res["pcqm_contact_b256"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
