#!/usr/bin/env python3
"""Block-diagonal multi-head self-attention (graph_hscn/nn/functional.py SelfAttentionFn, csrc/attention.hip): forward
plus backward of the operator on 1024 Peptides-shaped graphs in 8 batches of 128 at (heads, dh) = (4, 4), (4, 16),
(4, 24), (8, 8), and once on 32 graphs each of the PascalVOC-SP and PCQM-Contact shapes at (4, 16).  The input is a
random float32 qkv [N, 3D] on the graphs' node ranges.  Read-only towards the package.

Three candidates, alternated window by window in one process, on the same device batches:
* ``hip``: the operator -- one forward launch, two backward launches, nothing padded;
* ``sdpa``: what a user writes with torch-ROCm ops: ``to_dense_batch``-style padding of q, k, v to [B, heads, n_max, dh]
  (index_copy), ``F.scaled_dot_product_attention`` with the key mask, gather of the valid rows, autograd backward;
* ``mha``: ``torch.nn.MultiheadAttention(batch_first=True)`` with ``key_padding_mask`` on the padded [B, n_max, D]
  input (it includes MHA's own two projections, which the other two do not: it is context, not the bar).

Timing: a host clock around a window of passes over the batches that ends in one device synchronise, after a warm-up
pass; a window is at least ``--reps`` passes and at least 50 ms of the fastest candidate (the same count for all
candidates of a case, recorded as "reps"); ``--windows`` windows per number (default 9, at least 7), the median per pass with the spread (max - min) /
median.  Peak device memory of one forward + backward pass per candidate (``torch.cuda.max_memory_allocated`` above
the resident inputs).  Writes profiles/attention_bench.json (--out)."""
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

from graph_hscn import _hip
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.nn import functional as Fh

DEV = "cuda"


MIN_WINDOW_SECONDS = 0.05     # a window shorter than this measures the clock and the scheduler, not the work


def windows(fns, n, reps):
    """``reps`` is a floor: it is raised, for all candidates alike, until the fastest candidate's window lasts at
    least MIN_WINDOW_SECONDS (calibrated on one timed pass after the warm-up pass)."""
    fastest = float("inf")
    for f in fns.values():
        f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        fastest = min(fastest, time.perf_counter() - t0)
    reps = max(reps, int(MIN_WINDOW_SECONDS / fastest) + 1)
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


def peak_bytes(f):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


class Item:
    """One batch's node ranges, its padding map and a random qkv / cotangent at width D."""

    def __init__(self, b, heads, dh, g):
        D = heads * dh
        self.N, self.B, self.n_max = int(b.num_nodes), int(b.num_graphs), int(b.max_nodes)
        self.ptr32 = b.ptr32.to(DEV)
        ptr = b.ptr.to(DEV)
        sizes = ptr[1:] - ptr[:-1]
        graph = torch.repeat_interleave(torch.arange(self.B, device=DEV), sizes)
        self.rows = graph * self.n_max + (torch.arange(self.N, device=DEV) - ptr[graph])     # row of node i when padded
        self.valid = torch.zeros(self.B * self.n_max, dtype=torch.bool, device=DEV)
        self.valid[self.rows] = True
        self.valid = self.valid.view(self.B, self.n_max)
        self.qkv = torch.randn(self.N, 3 * D, generator=g).to(DEV).requires_grad_(True)
        self.x = torch.randn(self.N, D, generator=g).to(DEV).requires_grad_(True)
        self.g_out = torch.randn(self.N, D, generator=g).to(DEV)


def operator_case(batches, heads, dh, a, reps):
    D = heads * dh
    g = torch.Generator().manual_seed(100 * heads + dh)
    items = [Item(b, heads, dh, g) for b in batches]
    mha = torch.nn.MultiheadAttention(D, heads, batch_first=True).to(DEV)

    def hip_fwd(it):
        return Fh.SelfAttentionFn.apply(it.qkv, it.ptr32, it.n_max, heads)

    def sdpa_fwd(it):
        dense = it.qkv.new_zeros(it.B * it.n_max, 3 * D).index_copy(0, it.rows, it.qkv)
        q, k, v = (t.reshape(it.B, it.n_max, heads, dh).transpose(1, 2) for t in dense.split(D, 1))
        o = TF.scaled_dot_product_attention(q, k, v, attn_mask=it.valid[:, None, None, :])
        return o.transpose(1, 2).reshape(it.B * it.n_max, D)[it.rows]

    def mha_fwd(it):
        dense = it.x.new_zeros(it.B * it.n_max, D).index_copy(0, it.rows, it.x).view(it.B, it.n_max, D)
        y, _ = mha(dense, dense, dense, key_padding_mask=~it.valid, need_weights=False)
        return y.reshape(it.B * it.n_max, D)[it.rows]

    def both(fwd, leaf):
        def run():
            for it in items:
                torch.autograd.grad(fwd(it), [getattr(it, leaf)], it.g_out)
        return run

    it0 = items[0]
    oh, os_ = hip_fwd(it0), sdpa_fwd(it0)
    gh = torch.autograd.grad(oh, [it0.qkv], it0.g_out)[0]
    gs = torch.autograd.grad(os_, [it0.qkv], it0.g_out)[0]
    row = {"heads": heads, "dh": dh, "D": D, "nodes": sum(it.N for it in items), "batches": len(items),
           "largest_graph": max(it.n_max for it in items),
           "padded_rows": sum(it.B * it.n_max for it in items),
           "max_abs_difference_hip_vs_sdpa": {"out": float((oh - os_).abs().max()), "g_qkv": float((gh - gs).abs().max())}}
    fns = {"hip": both(hip_fwd, "qkv"), "sdpa": both(sdpa_fwd, "qkv"), "mha": both(mha_fwd, "x")}
    row["forward_backward"] = windows(fns, a.windows, reps)
    one = {"hip": lambda: torch.autograd.grad(hip_fwd(it0), [it0.qkv], it0.g_out),
           "sdpa": lambda: torch.autograd.grad(sdpa_fwd(it0), [it0.qkv], it0.g_out),
           "mha": lambda: torch.autograd.grad(mha_fwd(it0), [it0.x], it0.g_out)}
    row["peak_bytes_one_batch_forward_backward"] = {k: peak_bytes(f) for k, f in one.items()}
    fb = row["forward_backward"]
    row["sdpa_over_hip"] = fb["sdpa"]["seconds_per_pass"] / fb["hip"]["seconds_per_pass"]
    row["mha_over_hip"] = fb["mha"]["seconds_per_pass"] / fb["hip"]["seconds_per_pass"]
    return row


def device_batches(name, graphs, batch):
    gs = make_dataset(name, graphs, seed=0)
    return [Batch.from_data_list(gs[i:i + batch]).to(DEV) for i in range(0, graphs, batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py measures on the HIP device: none found")
    res = {"device": torch.cuda.get_device_name(0), "graphs": a.graphs, "batch": a.batch,
           "tile": int(_hip.lib().hscn_attention_tile()), "chunk": int(_hip.lib().hscn_attention_chunk())}
    pep = device_batches("peptides_func", a.graphs, a.batch)
    for heads, dh in ((4, 4), (4, 16), (4, 24), (8, 8)):
        key = f"peptides_h{heads}_dh{dh}"
        res[key] = operator_case(pep, heads, dh, a, a.reps)
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    for name in ("pascalvoc_sp_node", "pcqm_contact_link"):
        key = f"{name}_h4_dh16"
        res[key] = operator_case(device_batches(name, 32, 32), 4, 16, a, a.reps)
        print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
