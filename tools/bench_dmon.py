#!/usr/bin/env python3
"""DMoN pooling's launch pair (hscn_dmon_sparse_fwd + hscn_dmon_sparse_bwd, csrc/dmon.hip) beside MinCUT's
(hscn_mincut_sparse_fwd + hscn_mincut_sparse_bwd, csrc/mincut.hip) on the same tensors in the same process: one
batch of 128 graphs at Peptides-func shape with K = 16 clusters and one at PascalVOC-SP shape with K = 64, the edge
list after gcn_norm(add_self_loops=True) as the SCN hands it over, logits N(0, 2^2), x = 16 random hidden features.
Read-only towards the package.

The yardstick is MinCUT's pair in the same run: DMoN streams the same S, CSR and X once plus O(n K) extra arithmetic.
Per shape: forward + backward of both, forward alone and backward alone; the DMoN / MinCUT ratio with the spread of
either timing; the algorithmic bytes of DMoN's pair computed from the shapes and the ACHIEVED bytes/s (algorithmic
bytes / measured time; not a hardware counter).

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the two candidates take turns window by
window, ``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) /
median.

Every shape is measured by a child process of its own under a time limit (``--limit`` seconds); the parent never opens
the device, and a child that fails or runs out of time ends the run: nothing is started after it.  Writes
profiles/dmon_bench.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

CASES = {"peptides_func": 16, "pascalvoc_sp": 64}
FX = 16


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


def measure(name, a):
    import torch
    from graph_hscn import _hip
    from graph_hscn._hip import ptr, stream
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.nn.functional import DMON_STATS
    from graph_hscn.nn.pool import gcn_norm
    from graph_hscn.structure import Relation
    if not torch.cuda.is_available():
        raise SystemExit("bench_dmon.py measures on the HIP device: none found")
    dev, K = "cuda", CASES[name]
    big = Batch.from_data_list(make_dataset(name, a.batch, seed=0))
    N, G = int(big.num_nodes), a.batch
    ei, _ = gcn_norm(big.edge_index.to(dev), None, N, add_self_loops=True)
    E = int(ei.size(1))
    rel = Relation(ei, N, N)
    r, c = rel.csr_t, rel.csr
    nptr = big.ptr.to(dev).to(torch.int32).contiguous()
    g = torch.Generator().manual_seed(K)
    logits = (torch.randn(N, K, generator=g) * 2).to(dev)
    x = torch.randn(N, FX, generator=g).to(dev)
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    S, ss, px, padj, gl_out = new(N, K), new(G, K, K), new(G, K, FX), new(G, K, K), new(N, K)
    d_stats, d_vec, d_losses, d_gl = new(G, DMON_STATS), new(G, 2, K), new(3), torch.ones(3, device=dev)
    m_stats, m_losses, m_gl = new(G, 4), new(2), torch.ones(2, device=dev)
    st = stream()

    def dmon_fwd():
        _hip.call("hscn_dmon_sparse_fwd", ptr(logits), ptr(x), ptr(r.rowptr), ptr(r.col), ptr(nptr), ptr(S), ptr(d_stats),
                  ptr(ss), ptr(d_vec), ptr(px), ptr(padj), ptr(d_losses), N, G, K, FX, st)

    def dmon_bwd():
        _hip.call("hscn_dmon_sparse_bwd", ptr(S), ptr(d_stats), ptr(ss), ptr(d_vec), ptr(r.rowptr), ptr(r.col),
                  ptr(c.rowptr), ptr(c.col), ptr(nptr), ptr(d_gl), ptr(gl_out), N, G, K, st)

    def mincut_fwd():
        _hip.call("hscn_mincut_sparse_fwd", ptr(logits), ptr(x), ptr(r.rowptr), ptr(r.col), ptr(nptr), ptr(S),
                  ptr(m_stats), ptr(ss), ptr(px), ptr(padj), ptr(m_losses), N, G, K, FX, st)

    def mincut_bwd():
        _hip.call("hscn_mincut_sparse_bwd", ptr(S), ptr(m_stats), ptr(ss), ptr(r.rowptr), ptr(r.col), ptr(c.rowptr),
                  ptr(c.col), ptr(nptr), ptr(m_gl), ptr(gl_out), N, G, K, st)

    def pair(f, b):
        return lambda: (f(), b())

    row = {"shape": name, "graphs": G, "K": K, "Fx": FX, "nodes": N, "edges_with_self_loops": E,
           "largest_graph": int(big.max_nodes)}
    row["forward_backward"] = windows({"dmon": pair(dmon_fwd, dmon_bwd), "mincut": pair(mincut_fwd, mincut_bwd)},
                                      a.windows, a.reps)
    row["forward"] = windows({"dmon": dmon_fwd, "mincut": mincut_fwd}, a.windows, a.reps)
    mincut_fwd()                      # the backward alone reads its own operator's statistics
    row["backward"] = {}
    row["backward"].update(windows({"mincut": mincut_bwd}, a.windows, a.reps))
    dmon_fwd()
    row["backward"].update(windows({"dmon": dmon_bwd}, a.windows, a.reps))
    torch.cuda.synchronize()
    if not all(bool(torch.isfinite(t).all()) for t in (d_losses, d_stats, gl_out, m_losses)):
        raise SystemExit("bench_dmon.py: a non-finite result")
    for k in ("forward_backward", "forward", "backward"):
        d, m = row[k]["dmon"], row[k]["mincut"]
        row[k]["dmon_over_mincut"] = d["seconds"] / m["seconds"]
        # the run-to-run spread of the MinCUT timing itself is the yardstick for the ratio
        row[k]["ratio_beyond_mincut_spread"] = bool(abs(d["seconds"] - m["seconds"]) > m["spread"] * m["seconds"])
    # algorithmic bytes of DMoN's pair, from the shapes: the softmax reads the logits and writes S; the statistics kernel
    # reads S once per node and once per edge, X, rowptr + col, node_ptr, and writes the per-graph blocks; the backward
    # reads S once per node and once per edge in either direction, both CSRs, ss + vec + the statistics row, and writes
    # g_logits
    fwd = 4 * (2 * N * K + N * K + E * K + N * FX + (N + 1) + E + (G + 1) + G * (2 * K * K + K * FX + 2 * K + DMON_STATS) + 3)
    bwd = 4 * (N * K + 2 * E * K + 2 * (N + 1) + 2 * E + (G + 1) + G * (K * K + 2 * K + DMON_STATS) + 3 + N * K)
    row["algorithmic_bytes"] = {"forward": fwd, "backward": bwd, "forward_backward": fwd + bwd}
    row["achieved_bytes_per_s"] = {"forward": fwd / row["forward"]["dmon"]["seconds"],
                                   "backward": bwd / row["backward"]["dmon"]["seconds"],
                                   "forward_backward": (fwd + bwd) / row["forward_backward"]["dmon"]["seconds"]}
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dmon_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--case", choices=sorted(CASES), help="(child) measure this shape and print its JSON row")
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if a.case:
        print(json.dumps(measure(a.case, a)))
        return
    res = {"batch": a.batch, "windows": a.windows, "reps": a.reps, "shapes": {}}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--windows", str(a.windows), "--reps",
               str(a.reps), "--batch", str(a.batch)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_dmon.py: {name} exceeded {a.limit} s; nothing further was started")
        if done.returncode != 0:
            raise SystemExit(f"bench_dmon.py: {name} ended with status {done.returncode}; nothing further was started")
        res["shapes"][name] = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(json.dumps({name: res["shapes"][name]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
