#!/usr/bin/env python3
"""GINEConv's aggregate (graph_hscn/nn/functional.py GINEAggregateFn, csrc/gine.hip) on 1024 Peptides-shaped graphs with
edge features (``make_dataset(..., edge_features=True)``, De = 3) in batches of 128, at F = 16 and F = 64 (random
float32 node features of that width on the graphs' structure).  Read-only towards the package.

Two candidates, alternated window by window in one process, on the same device batches:
* ``hip``: the operator -- one forward launch; backward = source walk (gx) + per-edge gm + ``hscn_linear_bwd_w``;
* ``torch``: the same operator written with torch-ROCm ops, what a user has to write without it: ``F.linear`` for lin,
  ``index_select``, ``+``, ``relu``, ``index_add_``, autograd for the backward.

Per width: forward + backward of both (the bar: ``hip`` faster by more than the larger of the two spreads), forward
alone and backward alone, the algorithmic bytes of a forward and of a forward + backward computed from the shapes and
the ACHIEVED bytes/s (algorithmic bytes / measured time; not a hardware counter).  For context, one training iteration
(forward, criterion, backward, Adam) of the 3-layer ``gine`` MPNN beside the 3-layer ``gcn`` MPNN, layered engine,
hidden width 16, the same batches.

Timing: a host clock around ``--reps`` passes over the 8 batches that end in one device synchronise, after a warm-up
pass; ``--windows`` windows per number (default 9, at least 7), the median per pass with the spread (max - min) /
median.  Writes profiles/gine_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch
import torch.nn.functional as TF

from graph_hscn.config.config import ACT_DICT, CONV_DICT
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.mpnn import MPNN
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import Relation
from graph_hscn.train import batching

DEV = "cuda"
DE = 3


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


def torch_aggregate(x, ea, W, b, src, dst, eps=0.0):
    m = torch.relu(x.index_select(0, src) + TF.linear(ea, W, b))
    return ((1.0 + eps) * x).index_add_(0, dst, m)


def operator_case(dev_batches, F, a):
    g = torch.Generator().manual_seed(F)
    items = []
    for b in dev_batches:
        N, E = int(b.num_nodes), int(b.edge_index.size(1))
        x = torch.randn(N, F, generator=g).to(DEV).requires_grad_(True)
        gz = torch.randn(N, F, generator=g).to(DEV)
        rel = Relation(b.edge_index, N, N, both=True)
        items.append((x, b.edge_attr, rel, b.edge_index[0].contiguous(), b.edge_index[1].contiguous(), gz, N, E))
    W = (torch.randn(F, DE, generator=g) / DE ** 0.5).to(DEV).requires_grad_(True)
    bias = (0.1 * torch.randn(F, generator=g)).to(DEV).requires_grad_(True)

    def hip_fwd(it):
        return Fh.GINEAggregateFn.apply(it[0], it[1], W, bias, it[2], 0.0)

    def torch_fwd(it):
        return torch_aggregate(it[0], it[1], W, bias, it[3], it[4])

    def both(fwd):
        def run():
            for it in items:
                torch.autograd.grad(fwd(it), [it[0], W, bias], it[5])
        return run

    def fwd_only(fwd):
        def run():
            with torch.no_grad():
                for it in items:
                    fwd(it)
        return run

    # the two candidates compute the same thing (different summation orders)
    zh, zt = hip_fwd(items[0]), torch_fwd(items[0])
    gh = torch.autograd.grad(zh, [items[0][0], W, bias], items[0][5])
    gt = torch.autograd.grad(zt, [items[0][0], W, bias], items[0][5])
    agree = {"z": float((zh - zt).abs().max()), "gx": float((gh[0] - gt[0]).abs().max()),
             "gW_rel": float((gh[1] - gt[1]).abs().max() / gt[1].abs().max())}
    row = {"F": F, "De": DE, "max_abs_difference_hip_vs_torch": agree}
    row["forward_backward"] = windows({"hip": both(hip_fwd), "torch": both(torch_fwd)}, a.windows, a.reps)
    row["forward"] = windows({"hip": fwd_only(hip_fwd), "torch": fwd_only(torch_fwd)}, a.windows, a.reps)

    def bwd_only(fwd):
        def run():
            for it, z in zip(items, run.outs):
                torch.autograd.grad(z, [it[0], W, bias], it[5], retain_graph=True)
        run.outs = [fwd(it) for it in items]
        return run
    row["backward"] = windows({"hip": bwd_only(hip_fwd), "torch": bwd_only(torch_fwd)}, a.windows, a.reps)
    fb = row["forward_backward"]
    th, tt = fb["hip"]["seconds_per_pass"], fb["torch"]["seconds_per_pass"]
    margin = max(fb["hip"]["spread"] * th, fb["torch"]["spread"] * tt)
    row["torch_over_hip"] = tt / th
    row["bar_hip_faster_by_more_than_the_larger_spread"] = bool(tt - th > margin)
    # algorithmic bytes of one pass over the set, from the shapes: forward = x read once as the self term and once per
    # edge, edge_attr, col + eid, rowptr, z written; backward adds the source walk (gz in place of x, x_j once per row)
    # and the per-edge pass (x[src], gz[dst], edge_attr, edge_index int64, gm written) plus gm and edge_attr read once
    # by the weight-gradient reduction
    N = sum(it[6] for it in items)
    E = sum(it[7] for it in items)
    fwd_bytes = 4 * (2 * N * F + E * F + E * DE + 2 * E + N)
    bwd_bytes = 4 * (3 * N * F + E * F + E * DE + 2 * E + N) + 4 * (3 * E * F + E * DE + 4 * E) + 4 * (E * F + E * DE)
    row["nodes"], row["edges"] = N, E
    row["algorithmic_bytes"] = {"forward": fwd_bytes, "forward_backward": fwd_bytes + bwd_bytes}
    row["achieved_bytes_per_s"] = {"forward": fwd_bytes / row["forward"]["hip"]["seconds_per_pass"],
                                   "forward_backward": (fwd_bytes + bwd_bytes) / th}
    return row


def model_case(dev_batches, a):
    out = {}
    fns = {}
    for name in ("gine", "gcn"):
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
    out["gine_over_gcn"] = (out["train_iteration_pass"]["gine"]["seconds_per_pass"]
                            / out["train_iteration_pass"]["gcn"]["seconds_per_pass"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gine_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if not torch.cuda.is_available():
        raise SystemExit("bench_gine.py measures on the HIP device: none found")
    graphs = make_dataset("peptides_func", a.graphs, seed=0, edge_features=True)
    probe = MPNN(CONV_DICT["gine"], ACT_DICT["relu"], 9, 16, 10, 3)
    dev = [batching.to_device(probe, Batch.from_data_list(graphs[i:i + a.batch]), DEV)
           for i in range(0, a.graphs, a.batch)]
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "batch": a.batch, "batches": len(dev),
           "long_row": Fh.GINE_LONG_ROW, "chunk": Fh.GINE_CHUNK}
    for F in (16, 64):
        res[f"aggregate_F{F}"] = operator_case(dev, F, a)
        print(json.dumps({f"aggregate_F{F}": res[f"aggregate_F{F}"]}), file=sys.stderr, flush=True)
    res["mpnn_3_layers_H16"] = model_case(dev, a)
    print(json.dumps({"mpnn_3_layers_H16": res["mpnn_3_layers_H16"]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
