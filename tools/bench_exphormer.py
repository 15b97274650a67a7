#!/usr/bin/env python3
"""Exphormer's typed sparse attention (nn.functional.ExphormerAttentionFn: hscn_exph_attn_fwd, _bwd_dst, _bwd_src,
_bwd_type, csrc/exphormer.hip) beside two yardsticks on the same batch in the same process.  Read-only towards the
package.

Shapes: one Peptides-func-shaped batch of 128 graphs, width 64, 4 heads, expander degree 6, the local edges with
feature rows of their own, and nv = 0, 1 or 4 virtual nodes per graph (nv0 / nv1 / nv4).

Yardsticks, taking turns with the operator window by window:
  torch      the same arithmetic composed of torch device ops on the materialised [E_union, HC] edge features:
             ``torch.cat([e_edge, e_type])[erow]`` (index_select), ``exp``, ``index_add_`` (scatter_add) -- what a user
             would write; its backward is autograd's (index_add / index_select backward: float atomics)
  dense      nn.functional.SelfAttentionFn, the per-graph dense attention (csrc/attention.hip), on the packed [N, 3 HC]
             projection of the same batch (real nodes only)
No ratio is promised; the table is what it is.  All three run through autograd: forward under ``torch.no_grad()``,
forward + backward with gradients for every float input.

Per shape: the medians with their spreads, and the algorithmic bytes of the operator's launches computed from the shapes
over the measured time as a share of the HBM peak -- ALGORITHMIC bytes / measured time, not a hardware counter; rows
gathered through the caches count once per edge and the type table once per launch.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the candidates take turns window by window,
``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) / median.
Every shape is measured by a child process of its own under a time limit (``--limit`` seconds); the parent never opens
the device, and a child that fails or runs out of time ends the run: nothing is started after it.  Writes
profiles/exphormer_bench.json (--out)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

WIDTH, HEADS, DEGREE = 64, 4, 6
CASES = {"nv0": 0, "nv1": 1, "nv4": 4}
HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s


def windows(fns, n, reps):
    """``fns``: {name: callable issuing ONE call sequence}; the candidates take turns.  {name: seconds per call}."""
    import torch
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    s = {k: [] for k in fns}
    for _ in range(n):
        for k, f in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                f()
            t1.record()
            t1.synchronize()
            s[k].append(t0.elapsed_time(t1) * 1e-3 / reps)
    out = {}
    for k, v in s.items():
        med = statistics.median(v)
        out[k] = {"seconds": med, "spread": (max(v) - min(v)) / med, "windows": n, "reps": reps}
    return out


def algorithmic_bytes(rows, E, El, T, typed, chunks, heads, HC):
    """What the operator's launches must move, from the shapes alone (4-byte words; int64 edge ends count two):
    forward: rowptr, (col, eid, erow) and the k and v rows per edge, every e_edge row once, the table once, q, out, Z;
    target pass: the same gathers, q / dout / out, Z, delta, dq, de_edge; source pass: k / v, per edge q and dout rows,
    Z and delta, dk, dv; type pass: per typed edge its id, two ends, four rows, Z and delta, the partials out and in."""
    e = El * HC + T * HC
    fwd = 4 * ((rows + 1) + 3 * E + 2 * E * HC + e + 2 * rows * HC + rows * heads)
    dst = 4 * ((rows + 1) + 3 * E + 2 * E * HC + e + 4 * rows * HC + 2 * rows * heads + El * HC)
    src = 4 * ((rows + 1) + 3 * E + 2 * E * HC + e + 4 * rows * HC + 2 * E * heads)
    typ = 4 * ((T + 1) + 5 * typed + 4 * typed * HC + 2 * typed * heads + 2 * chunks * HC + 2 * T * HC)
    return {"forward": fwd, "backward": dst + src + typ, "forward_backward": fwd + dst + src + typ}


def measure(name, a):
    import torch
    from graph_hscn import _hip
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.nn import functional as Fh
    from graph_hscn.structure import ExphormerStructure
    if not torch.cuda.is_available():
        raise SystemExit("bench_exphormer.py measures on the HIP device: none found")
    dev = "cuda"
    nv = CASES[name]
    big = Batch.from_data_list(make_dataset("peptides_func", a.batch, seed=0)).to(dev)
    N, B = int(big.num_nodes), int(big.num_graphs)
    struct = ExphormerStructure.of(big, DEGREE, nv, True, 0, edge_features=True)
    Fh.check_expander(dev)
    rows, E, El, T = struct.num_rows, struct.num_edges, struct.num_edge_rows, struct.num_types
    HC, C = WIDTH, WIDTH // HEADS
    g = torch.Generator().manual_seed(nv)
    rand = lambda *s, sd=1.0: (torch.randn(*s, generator=g) * sd).to(dev).requires_grad_(True)      # noqa: E731
    q, k, v, e_edge, e_type = rand(rows, HC), rand(rows, HC), rand(rows, HC), rand(El, HC, sd=0.5), rand(T, HC, sd=0.5)
    go = torch.randn(rows, HC, generator=g).to(dev)
    qkv, go_dense = rand(N, 3 * HC), torch.randn(N, HC, generator=g).to(dev)
    leaves = (q, k, v, e_edge, e_type, qkv)
    src, dst, erow = struct.edge_index[0], struct.edge_index[1], struct.erow.long()
    scale = 1.0 / math.sqrt(C)

    def hip():
        return Fh.ExphormerAttentionFn.apply(q, k, v, e_edge, e_type, struct, HEADS)

    def composed():
        ee = torch.cat([e_edge, e_type], 0).index_select(0, erow).view(E, HEADS, C)
        s = (q.index_select(0, dst).view(E, HEADS, C) * k.index_select(0, src).view(E, HEADS, C) * ee).sum(-1) * scale
        w = torch.exp(s.clamp(-5.0, 5.0))
        z = torch.zeros(rows, HEADS, device=dev).index_add_(0, dst, w)
        num = torch.zeros(rows, HEADS, C, device=dev).index_add_(0, dst, w.unsqueeze(-1) * v.index_select(0, src).view(E, HEADS, C))
        return (num / (z + 1e-6).unsqueeze(-1)).reshape(rows, HC)

    def dense():
        return Fh.SelfAttentionFn.apply(qkv, big.ptr32, int(big.max_nodes), HEADS)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f, cot):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(cot)
        return run

    with torch.no_grad():
        worst = float((hip() - composed()).abs().max())
    if not worst < 1e-4:
        raise SystemExit(f"bench_exphormer.py: the operator and the composed torch ops differ by {worst}")
    deg = struct.rel.csr.rowptr[1:] - struct.rel.csr.rowptr[:-1]
    trowptr, _ = struct.type_slots
    counts = (trowptr[1:] - trowptr[:-1]).tolist()
    L = _hip.lib()
    long_row, chunk = L.hscn_exph_type_long_row(), L.hscn_exph_type_chunk()
    chunks = sum(0 if c == 0 else (1 if c <= long_row else -(-c // chunk)) for c in counts)
    row = {"shape": name, "graphs": B, "heads": HEADS, "head_dim": C, "width": HC, "expander_degree": DEGREE,
           "virtual_nodes_per_graph": nv, "nodes": N, "rows": rows, "local_edges": El, "union_edges": E, "types": T,
           "typed_edges": int(sum(counts)), "largest_in_degree": int(deg.max()), "mean_in_degree": float(deg.float().mean()),
           "rows_beyond_long_row": int((deg > L.hscn_exph_attn_long_row()).sum()),
           "max_abs_difference_to_composed_forward": worst}
    row["forward"] = windows({"exphormer": fwd(hip), "torch": fwd(composed), "dense": fwd(dense)}, a.windows, a.reps)
    row["forward_backward"] = windows({"exphormer": fwd_bwd(hip, go), "torch": fwd_bwd(composed, go),
                                       "dense": fwd_bwd(dense, go_dense)}, a.windows, a.reps)
    fwd_bwd(hip, go)()
    torch.cuda.synchronize()
    Fh.check_attention(dev)
    if not all(bool(torch.isfinite(t.grad).all()) for t in leaves[:5]) or int(struct.rel.csr.flag.item()) != 0:
        raise SystemExit("bench_exphormer.py: a non-finite gradient or a flagged slot")
    for key in ("forward", "forward_backward"):
        for other in ("torch", "dense"):
            ours, ya = row[key]["exphormer"], row[key][other]
            row[key][f"exphormer_over_{other}"] = ours["seconds"] / ya["seconds"]
            # the run-to-run spread of the yardstick's timing itself is the yardstick for the ratio
            row[key][f"ratio_beyond_{other}_spread"] = bool(abs(ours["seconds"] - ya["seconds"]) > ya["spread"] * ya["seconds"])
    nbytes = algorithmic_bytes(rows, E, El, T, int(sum(counts)), chunks, HEADS, HC)
    row["algorithmic_bytes"] = nbytes
    row["materialised_edge_feature_bytes"] = 4 * E * HC
    row["algorithmic_bytes_over_time_share_of_hbm_peak"] = {
        key: nbytes[key] / row[key]["exphormer"]["seconds"] / HBM_PEAK_BYTES_PER_S for key in ("forward", "forward_backward")}
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exphormer_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--case", choices=sorted(CASES), help="(child) measure this shape and print its JSON row")
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if a.case:
        print(json.dumps(measure(a.case, a)))
        return
    res = {"batch": a.batch, "windows": a.windows, "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "shapes": {}}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--windows", str(a.windows), "--reps",
               str(a.reps), "--batch", str(a.batch)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_exphormer.py: {name} exceeded {a.limit} s; nothing further was started")
        if done.returncode != 0:
            raise SystemExit(f"bench_exphormer.py: {name} ended with status {done.returncode}; nothing further was "
                             "started")
        res["shapes"][name] = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(json.dumps({name: res["shapes"][name]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
