#!/usr/bin/env python3
"""GatedGCN's aggregate (graph_hscn/nn/functional.py GatedGCNAggregateFn, csrc/gatedgcn.hip) on 1024 Peptides-shaped
graphs with edge features in batches of 128, at H = 16 and H = 64 (random float32 Ax, Bx, Dx, Ex [N, H] and Ce [E, H] on
the graphs' structure, all five with a gradient, cotangents on both outputs).  Read-only towards the package.

Two candidates, alternated window by window in one process, on the same device batches:
* ``hip``: the operator -- one forward launch; backward = the target-keyed pass + the source-keyed pass;
* ``torch``: the same operator composed from torch-ROCm ops with autograd, what a user has to write without it:
  ``index_select``, ``+``, ``sigmoid``, ``*``, two ``index_add_``, ``/``.

Per width: forward + backward of both (the bar, as tools/bench_gine.py states it: ``hip`` faster by more than the larger
of the two spreads), forward alone and backward alone, the algorithmic bytes of a forward and of a forward + backward
computed from the shapes and the ACHIEVED bytes/s (algorithmic bytes / measured time; not a hardware counter).  For
context, one training iteration (forward, criterion, backward, Adam) of the 3-layer ``gatedgcn`` MPNN beside the 3-layer
``gine`` MPNN, layered engine, hidden width 16, the same batches.

Timing: a host clock around ``--reps`` passes over the 8 batches that end in one device synchronise, after a warm-up
pass; ``--windows`` windows per number (default 9, at least 7), the median per pass with the spread (max - min) /
median.  Writes profiles/gatedgcn_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.mpnn import MPNN
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import Relation
from graph_hscn.train import batching

DEV = "cuda"


def windows(fns, n, reps, warm=True):
    """``fns``: {name: callable doing ONE pass}; the candidates take turns, window by window.  {name: seconds per pass}."""
    if warm:
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    s = {k: [] for k in fns}
    for _ in range(n):
        for k, f in fns.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            s[k].append((time.perf_counter() - t0) / reps)
    out = {}
    for k, v in s.items():
        med = statistics.median(v)
        out[k] = {"seconds_per_pass": med, "spread": (max(v) - min(v)) / med, "windows": n, "reps": reps}
    return out


def torch_aggregate(Ax, Bx, Dx, Ex, Ce, src, dst):
    e = Dx.index_select(0, dst) + Ex.index_select(0, src) + Ce
    s = torch.sigmoid(e)
    num = torch.zeros_like(Ax).index_add_(0, dst, s * Bx.index_select(0, src))
    den = torch.zeros_like(Ax).index_add_(0, dst, s)
    return Ax + num / (den + 1e-6), e


def operator_case(dev_batches, H, a):
    g = torch.Generator().manual_seed(H)
    items = []
    for b in dev_batches:
        N, E = int(b.num_nodes), int(b.edge_index.size(1))
        leaves = [torch.randn(N, H, generator=g).to(DEV).requires_grad_(True) for _ in range(2)]
        leaves += [(0.7 * torch.randn(N, H, generator=g)).to(DEV).requires_grad_(True) for _ in range(2)]
        leaves.append((0.7 * torch.randn(E, H, generator=g)).to(DEV).requires_grad_(True))
        cot = (torch.randn(N, H, generator=g).to(DEV), torch.randn(E, H, generator=g).to(DEV))
        rel = Relation(b.edge_index, N, N, both=True)
        items.append((leaves, rel, b.edge_index[0].contiguous(), b.edge_index[1].contiguous(), cot, N, E))

    def hip_fwd(it):
        return Fh.GatedGCNAggregateFn.apply(*it[0], it[1])

    def torch_fwd(it):
        return torch_aggregate(*it[0], it[2], it[3])

    def both(fwd):
        def run():
            for it in items:
                torch.autograd.grad(fwd(it), it[0], it[4])
        return run

    def fwd_only(fwd):
        def run():
            with torch.no_grad():
                for it in items:
                    fwd(it)
        return run

    # the two candidates compute the same thing (different summation orders)
    oh, ot = hip_fwd(items[0]), torch_fwd(items[0])
    gh = torch.autograd.grad(oh, items[0][0], items[0][4])
    gt = torch.autograd.grad(ot, items[0][0], items[0][4])
    agree = {"h": float((oh[0] - ot[0]).abs().max()), "e": float((oh[1] - ot[1]).abs().max())}
    agree.update({"g" + n: float((x - y).abs().max()) for n, x, y in zip(("Ax", "Bx", "Dx", "Ex", "Ce"), gh, gt)})
    row = {"H": H, "max_abs_difference_hip_vs_torch": agree}
    row["forward_backward"] = windows({"hip": both(hip_fwd), "torch": both(torch_fwd)}, a.windows, a.reps)
    row["forward"] = windows({"hip": fwd_only(hip_fwd), "torch": fwd_only(torch_fwd)}, a.windows, a.reps)

    def bwd_only(fwd):
        def run():
            for it, o in zip(items, run.outs):
                torch.autograd.grad(o, it[0], it[4], retain_graph=True)
        run.outs = [fwd(it) for it in items]
        return run
    row["backward"] = windows({"hip": bwd_only(hip_fwd), "torch": bwd_only(torch_fwd)}, a.windows, a.reps)
    fb = row["forward_backward"]
    th, tt = fb["hip"]["seconds_per_pass"], fb["torch"]["seconds_per_pass"]
    margin = max(fb["hip"]["spread"] * th, fb["torch"]["spread"] * tt)
    row["torch_over_hip"] = tt / th
    row["bar_hip_faster_by_more_than_the_larger_spread"] = bool(tt - th > margin)
    # algorithmic bytes of one pass over the set, from the shapes ("GatedGCN"):
    #   forward:      per node Ax, Dx read, h, den written; per edge Ex_j, Bx_j gathered, Ce read, e^ written; col + eid,
    #                 rowptr
    #   target pass:  per node gh, den, h, Ax read, gn, gDx written; per edge Bx_j, e^, its cotangent read, ge written
    #   source pass:  per node gBx, gEx written; per edge e^, gn_i, ge read
    N = sum(it[5] for it in items)
    E = sum(it[6] for it in items)
    fwd_bytes = 4 * (4 * N * H + 4 * E * H + 2 * E + N)
    bwd_bytes = 4 * (6 * N * H + 4 * E * H + 2 * E + N) + 4 * (2 * N * H + 3 * E * H + 2 * E + N)
    row["nodes"], row["edges"] = N, E
    row["algorithmic_bytes"] = {"forward": fwd_bytes, "forward_backward": fwd_bytes + bwd_bytes}
    row["achieved_bytes_per_s"] = {"forward": fwd_bytes / row["forward"]["hip"]["seconds_per_pass"],
                                   "forward_backward": (fwd_bytes + bwd_bytes) / th}
    return row


def model_case(dev_batches, a):
    out = {}
    fns = {}
    for name in ("gatedgcn", "gine"):
        torch.manual_seed(0)
        m = MPNN(CONV_DICT[name], ACT_DICT["relu"], 9, 16, 10, 3, dropout=0.0).to(DEV)
        with torch.no_grad():
            m(dev_batches[0])
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)

        def run(m=m, opt=opt):
            for b in dev_batches:
                opt.zero_grad(set_to_none=True)
                loss, _ = criterion("cross_entropy", m(b), b.y)
                loss.backward()
                opt.step()
        fns[name] = run
    out["train_iteration_pass"] = windows(fns, a.windows, max(1, a.reps // 2))
    out["gatedgcn_over_gine"] = (out["train_iteration_pass"]["gatedgcn"]["seconds_per_pass"]
                                 / out["train_iteration_pass"]["gine"]["seconds_per_pass"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatedgcn_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if not torch.cuda.is_available():
        raise SystemExit("bench_gatedgcn.py measures on the HIP device: none found")
    graphs = make_dataset("peptides_func", a.graphs, seed=0, edge_features=True)
    probe = MPNN(CONV_DICT["gatedgcn"], ACT_DICT["relu"], 9, 16, 10, 3)
    dev = [batching.to_device(probe, Batch.from_data_list(graphs[i:i + a.batch]), DEV)
           for i in range(0, a.graphs, a.batch)]
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "batch": a.batch, "batches": len(dev),
           "long_row": Fh.GATEDGCN_LONG_ROW, "chunk": Fh.GATEDGCN_CHUNK}
    for H in (16, 64):
        res[f"aggregate_H{H}"] = operator_case(dev, H, a)
        print(json.dumps({f"aggregate_H{H}": res[f"aggregate_H{H}"]}), file=sys.stderr, flush=True)
    res["mpnn_3_layers_H16"] = model_case(dev, a)
    print(json.dumps({"mpnn_3_layers_H16": res["mpnn_3_layers_H16"]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
