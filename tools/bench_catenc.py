#!/usr/bin/env python3
"""The categorical encoders (graph_hscn/nn/functional.py CategoricalEmbedFn, csrc/catenc.hip) on Peptides-shaped batches
of 128 graphs: the atom columns (n ~ 19 k nodes, F = 9, 174 table rows) and the bond columns (E ~ 39 k edges, F = 3,
13 table rows) at D = 16, 64 and 128.  Read-only towards the package.

Candidates, alternated window by window in one process, on the same device tensors:
* ``hip``: the operator -- one gather launch; backward = the ordered segment reduce over the cached CategoryIndex (the
  steady state of epochs over device-resident batches);
* ``hip_rebuild``: the same with the CategoryIndex built anew in every backward (a loader that hands over fresh
  tensors every step: the index build's four launches are part of each step);
* ``torch``: the same computation written with torch-ROCm ops and autograd, what a user has to write without the
  operator: F ``index_select`` s added in column order; its backward is ``index_add_`` with float atomics.

Per shape: forward, backward alone, forward + backward, and the index build by itself; ``torch_over_hip`` is the ratio
of the medians (>= 1: the operator is not slower).  The torch composition is the yardstick, not a target: a shape where
the ratio is below 1 is reported as such (``not_slower``: false).  The two candidates' gradients differ by summation
order only; the largest difference is recorded, as is whether two ``hip`` runs give the same bits and two ``torch``
runs do.

Timing: a host clock around ``--reps`` passes over the batches that end in one device synchronise, after a warm-up
pass; ``--windows`` windows per number (default 9, at least 7), the median per pass with the spread (max - min) /
median.  Writes profiles/catenc_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

from graph_hscn import structure
from graph_hscn.data import Batch
from graph_hscn.encoder import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.nn import functional as Fh

DEV = "cuda"


def windows(fns, n, reps):
    """``fns``: {name: callable doing ONE pass}; the candidates take turns, window by window.  {name: seconds per pass}."""
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


def ratio(row, name="hip"):
    th, tt = row[name]["seconds_per_pass"], row["torch"]["seconds_per_pass"]
    return {"torch_over_hip": tt / th, "not_slower": bool(tt >= th),
            "clear_of_both_spreads": bool(abs(tt - th) > max(row[name]["spread"] * th, row["torch"]["spread"] * tt))}


def shape_case(kind, tensors, cards, D, a):
    g = torch.Generator().manual_seed(D)
    R = sum(cards)
    W = (0.3 * torch.randn(R, D, generator=g)).to(DEV).requires_grad_(True)
    items = [(x, torch.randn(x.size(0), D, generator=g).to(DEV)) for x in tensors]

    def hip_fwd(x):
        return Fh.categorical_embed(W, x, cards)

    def torch_fwd(x):
        return Fh.categorical_embed_reference(W, x, cards)

    def fwd_only(fwd):
        def run():
            with torch.no_grad():
                for x, _ in items:
                    fwd(x)
        return run

    def both(fwd, rebuild=False):
        def run():
            for x, cot in items:
                if rebuild:
                    structure._CAT_CACHE.clear()
                torch.autograd.grad(fwd(x), W, cot)
        return run

    def bwd_only(fwd):
        def run():
            for (x, cot), o in zip(items, run.outs):
                torch.autograd.grad(o, W, cot, retain_graph=True)
        run.outs = [fwd(x) for x, _ in items]
        return run

    def index_only():
        for x, _ in items:
            structure.build_category_index(x, cards)

    x0, c0 = items[0]
    gh = [torch.autograd.grad(hip_fwd(x0), W, c0)[0] for _ in range(2)]
    gt = [torch.autograd.grad(torch_fwd(x0), W, c0)[0] for _ in range(2)]
    row = {"kind": kind, "D": D, "F": len(cards), "table_rows": R, "items_per_batch": [int(x.size(0)) for x, _ in items],
           "longest_table_row": int(torch.bincount(x0[:, 0]).max()),
           "forward_equal_bits": bool(torch.equal(hip_fwd(x0), torch_fwd(x0))),
           "max_abs_gradient_difference_hip_vs_torch": float((gh[0] - gt[0]).abs().max()),
           "two_hip_runs_same_bits": bool(torch.equal(gh[0], gh[1])),
           "two_torch_runs_same_bits": bool(torch.equal(gt[0], gt[1]))}
    row["forward"] = windows({"hip": fwd_only(hip_fwd), "torch": fwd_only(torch_fwd)}, a.windows, a.reps)
    row["backward"] = windows({"hip": bwd_only(hip_fwd), "torch": bwd_only(torch_fwd)}, a.windows, a.reps)
    row["forward_backward"] = windows({"hip": both(hip_fwd), "hip_rebuild": both(hip_fwd, True), "torch": both(torch_fwd)},
                                      a.windows, a.reps)
    row["index_build"] = windows({"hip": index_only}, a.windows, a.reps)
    row["ratios"] = {"forward": ratio(row["forward"]), "backward": ratio(row["backward"]),
                     "forward_backward": ratio(row["forward_backward"]),
                     "forward_backward_with_index_build": ratio(row["forward_backward"], "hip_rebuild")}
    Fh.check_categorical(DEV)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catenc_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if not torch.cuda.is_available():
        raise SystemExit("bench_catenc.py measures on the HIP device: none found")
    lib = Fh._hip.lib()
    graphs = make_dataset("peptides_func", a.graphs, seed=0, edge_features=True)
    batches = [Batch.from_data_list(graphs[i:i + a.batch]) for i in range(0, a.graphs, a.batch)]
    atoms = [b.x.to(DEV).contiguous() for b in batches]
    bonds = [b.edge_attr.to(DEV).contiguous() for b in batches]
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "batch": a.batch, "batches": len(batches),
           "long_row": int(lib.hscn_catenc_long_row()), "chunk": int(lib.hscn_catenc_chunk()),
           "sort_chunk": int(lib.hscn_catenc_sort_chunk()), "shapes": []}
    for kind, tensors, cards in (("atom", atoms, tuple(ATOM_FEATURE_DIMS)), ("bond", bonds, tuple(BOND_FEATURE_DIMS))):
        for D in (16, 64, 128):
            row = shape_case(kind, tensors, cards, D, a)
            res["shapes"].append(row)
            print(json.dumps({f"{kind}_D{D}": row["ratios"]}), file=sys.stderr, flush=True)
    res["not_slower_at_every_shape"] = {k: all(r["ratios"][k]["not_slower"] for r in res["shapes"])
                                        for k in ("forward", "backward", "forward_backward",
                                                  "forward_backward_with_index_build")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out, "not_slower_at_every_shape": res["not_slower_at_every_shape"]}))


if __name__ == "__main__":
    main()
