#!/usr/bin/env python3
"""Shortest-path attention bias (graph_hscn/nn/functional.py shortest_path_buckets / BiasedSelfAttentionFn, csrc/spd.hip,
csrc/attention.hip): three times per case, on the same device batches --
* ``buckets``: the bucket build of every batch (one launch per batch; in a model it runs once per batch object);
* ``biased``: forward plus backward of the biased operator (gradients for qkv and the table);
* ``unbiased``: forward plus backward of ``SelfAttentionFn`` on the same qkv, the same cotangent.
Cases: 1024 Peptides-func-shaped graphs in 8 batches of 128 at (heads, dh) = (4, 16) and (4, 24), and 32 PascalVOC-SP-
shaped graphs (n <= 500) in one batch at (4, 16); max_dist = 20 (21 buckets).  Read-only towards the package.

Timing (tools/bench_attention.py's): a host clock around a window of passes over the batches that ends in one device
synchronise, after a warm-up pass; the candidates alternate window by window in one process; a window is at least
``--reps`` passes and at least 50 ms of the fastest candidate; ``--windows`` windows per number (default 9, at least 7),
the median per pass with the spread (max - min) / median.  Also recorded: the bytes of bucket matrix a pass of each
biased kernel streams (heads x sum n^2 per kernel, three kernels) beside the qkv bytes.  Writes
profiles/attention_bias_bench.json (--out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd"), os.path.join(ROOT, "tools")]
import torch

from bench_attention import windows
from graph_hscn import _hip
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.nn import functional as Fh
from graph_hscn.train import batching

DEV = "cuda"
MAX_DIST = 20


def device_batches(name, graphs, batch):
    """Batches on the device the way the training loop moves them (their node counts stay on the host beside them)."""
    gs = make_dataset(name, graphs, seed=0)
    return [batching.to_device(None, Batch.from_data_list(gs[i:i + batch]), DEV) for i in range(0, graphs, batch)]


def case(batches, heads, dh, a):
    D = heads * dh
    g = torch.Generator().manual_seed(100 * heads + dh)
    items = []
    for b in batches:
        N = int(b.num_nodes)
        items.append({"b": b, "ptr32": b.ptr32, "mn": int(b.max_nodes), "spd": Fh.shortest_path_buckets(b, MAX_DIST),
                      "qkv": torch.randn(N, 3 * D, generator=g).to(DEV).requires_grad_(True),
                      "g_out": torch.randn(N, D, generator=g).to(DEV)})
    table = (0.02 * torch.randn(MAX_DIST + 1, heads, generator=g)).to(DEV).requires_grad_(True)
    Fh.check_spd(DEV)

    def buckets():
        for it in items:
            Fh.shortest_path_buckets(it["b"], MAX_DIST)

    def biased():
        for it in items:
            out = Fh.BiasedSelfAttentionFn.apply(it["qkv"], table, it["spd"], it["ptr32"], it["mn"], heads)
            torch.autograd.grad(out, [it["qkv"], table], it["g_out"])

    def unbiased():
        for it in items:
            out = Fh.SelfAttentionFn.apply(it["qkv"], it["ptr32"], it["mn"], heads)
            torch.autograd.grad(out, [it["qkv"]], it["g_out"])

    pairs = sum(int(it["spd"].bucket.numel()) for it in items)
    nodes = sum(int(it["qkv"].size(0)) for it in items)
    row = {"heads": heads, "dh": dh, "D": D, "max_dist": MAX_DIST, "batches": len(items), "nodes": nodes,
           "largest_graph": max(it["mn"] for it in items), "bucket_bytes": pairs,
           "bucket_bytes_streamed_per_pass": 3 * heads * pairs, "qkv_bytes": nodes * 3 * D * 4}
    row["times"] = windows({"buckets": buckets, "biased": biased, "unbiased": unbiased}, a.windows, a.reps)
    t = row["times"]
    row["biased_over_unbiased"] = t["biased"]["seconds_per_pass"] / t["unbiased"]["seconds_per_pass"]
    row["buckets_over_biased"] = t["buckets"]["seconds_per_pass"] / t["biased"]["seconds_per_pass"]
    Fh.check_attention(DEV)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bias_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_bias.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "batch": a.batch,
           "tile": int(_hip.lib().hscn_attention_tile()), "chunk": int(_hip.lib().hscn_attention_chunk())}
    pep = device_batches("peptides_func", a.graphs, a.batch)
    for heads, dh in ((4, 16), (4, 24)):
        key = f"peptides_h{heads}_dh{dh}"
        res[key] = case(pep, heads, dh, a)
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    key = "pascalvoc_sp_node_h4_dh16"
    res[key] = case(device_batches("pascalvoc_sp_node", 32, 32), 4, 16, a)
    print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
