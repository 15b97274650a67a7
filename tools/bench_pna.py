#!/usr/bin/env python3
"""The fused PNA aggregation (nn.functional.PNAAggregateFn: hscn_pna_fwd and the three backward launches,
csrc/pna.hip) beside the same arithmetic composed on the device from torch's ``index_add_`` and ``scatter_reduce``
(amax, amin), on the same batch in the same process.  Read-only towards the package.

Shape: one Peptides-func-shaped batch of 128 graphs, H = 64 columns, the four aggregators mean, min, max, std under the
three scalers identity, amplification, attenuation (GraphGPS's PNA configuration); ``a``, ``b`` [N, H] and ``t`` [E, H]
are drawn once, ``avg_deg_log`` is the batch's own.

Yardstick, taking turns with the operator window by window:
  composed   m = a[dst] + b[src] + t written as an [E, H] tensor, ``index_add_`` for the sum and the sum of squares,
             ``scatter_reduce`` amin / amax (``include_self=False``), the std, the three scalers and the concatenation:
             what the layer would be without the operator.  Its ties split the gradient evenly where the operator sends
             it to the first edge; random floats have no ties, so the two agree and the bench checks that they do.
Both run through autograd: forward under ``torch.no_grad()``, forward + backward with gradients for a, b and t.
No ratio is promised; the numbers are what they are.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the candidates take turns window by window,
``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) / median.
The measurement runs in a child process under a time limit (``--limit`` seconds); the parent never opens the device.
Writes profiles/pna_bench.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

H = 64
AGGREGATORS = ("mean", "min", "max", "std")
SCALERS = ("identity", "amplification", "attenuation")
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


def measure(a):
    import torch
    from graph_hscn.config.config import PNAConfig
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.nn import functional as Fh
    from graph_hscn.structure import Relation
    if not torch.cuda.is_available():
        raise SystemExit("bench_pna.py measures on the HIP device: none found")
    dev = "cuda"
    graphs = make_dataset("peptides_func", a.batch, seed=0)
    avg = PNAConfig.avg_deg_log_of(graphs)
    big = Batch.from_data_list(graphs).to(dev)
    ei = big.edge_index.contiguous()
    N, E = int(big.num_nodes), int(ei.size(1))
    rel = Relation(ei, N, N, both=True)
    g = torch.Generator().manual_seed(0)
    A_, B_, T_ = (torch.randn(N, H, generator=g).to(dev).requires_grad_(True),
                  torch.randn(N, H, generator=g).to(dev).requires_grad_(True),
                  torch.randn(E, H, generator=g).to(dev).requires_grad_(True))
    leaves = [A_, B_, T_]
    go = torch.randn(N, len(SCALERS) * len(AGGREGATORS) * H, generator=g).to(dev)
    src, dst = ei[0], ei[1]
    deg = torch.bincount(dst, minlength=N)
    cnt = deg.clamp(min=1).to(torch.float32).unsqueeze(1)
    lg = torch.log(cnt + 1)
    scales = [None, lg / avg, avg / lg]
    idx = dst.unsqueeze(1).expand(E, H)

    def fused():
        return Fh.PNAAggregateFn.apply(A_, B_, T_, rel, AGGREGATORS, SCALERS, avg)

    def composed():
        m = A_[dst] + B_[src] + T_
        total = torch.zeros(N, H, device=dev).index_add_(0, dst, m)
        mean = total / cnt
        mn = torch.zeros(N, H, device=dev).scatter_reduce(0, idx, m, "amin", include_self=False)
        mx = torch.zeros(N, H, device=dev).scatter_reduce(0, idx, m, "amax", include_self=False)
        msq = torch.zeros(N, H, device=dev).index_add_(0, dst, m * m) / cnt
        std = torch.sqrt(torch.relu(msq - mean * mean) + 1e-5)
        block = torch.cat([mean, mn, mx, std], 1)
        return torch.cat([block if s is None else block * s for s in scales], 1)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fwd_bwd(f):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(go)
        return run

    with torch.no_grad():
        ref = composed()
        worst = float((fused() - ref).abs().max() / ref.abs().max())
    if not worst < 1e-4:
        raise SystemExit(f"bench_pna.py: the operator and the composed ops differ by {worst} of the output's size")
    fwd_bwd(fused)()
    gf = [t.grad.clone() for t in leaves]
    fwd_bwd(composed)()
    gworst = max(float((a_ - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)) for a_, t in zip(gf, leaves))
    # (a guard against a wrong yardstick, not a test: the one-pass variance mean(m^2) - mean(m)^2 is ill-conditioned
    # where two messages of a node nearly agree, and among 1.3 M (node, column) pairs some do -- on this batch the
    # float32 restatement of tests/pna_oracle.py on the CPU is itself 2.6e-2 of the gradient's size from float64)
    if not gworst < 5e-2:
        raise SystemExit(f"bench_pna.py: the two backward passes differ by {gworst} of the gradient's size")
    row = {"graphs": int(big.num_graphs), "nodes": N, "edges": E, "H": H, "aggregators": list(AGGREGATORS),
           "scalers": list(SCALERS), "avg_deg_log": avg, "max_in_degree": int(deg.max().item()),
           "max_relative_difference_to_composed_forward": worst,
           "max_relative_difference_to_composed_gradients": gworst}
    row["forward"] = windows({"fused": fwd(fused), "composed": fwd(composed)}, a.windows, a.reps)
    row["forward_backward"] = windows({"fused": fwd_bwd(fused), "composed": fwd_bwd(composed)}, a.windows, a.reps)
    for key in ("forward", "forward_backward"):
        ours, ya = row[key]["fused"], row[key]["composed"]
        row[key]["fused_over_composed"] = ours["seconds"] / ya["seconds"]
        row[key]["ratio_beyond_composed_spread"] = bool(abs(ours["seconds"] - ya["seconds"]) > ya["spread"] * ya["seconds"])
    # forward: per edge one row of b and of t, per node a in, S A H out (no saved tensors under no_grad); backward: the
    # cotangent in, gw out, per edge b / gw (4 rows) / mean / arg (2 rows) / t in for each of the two walks, g_t out
    SA = len(SCALERS) * len(AGGREGATORS)
    f_bytes = 4 * (2 * E * H + N * H + N * SA * H)
    b_bytes = 4 * (N * SA * H + 5 * N * H + 2 * E * 9 * H + E * H + N * H)
    row["algorithmic_bytes"] = {"forward": f_bytes, "backward": b_bytes, "forward_backward": f_bytes + b_bytes + 4 * 4 * N * H}
    row["composed_intermediate_bytes"] = {"[E, H] messages": 4 * E * H, "[E, H] squares": 4 * E * H}
    row["algorithmic_bytes_over_time_share_of_hbm_peak"] = {
        key: row["algorithmic_bytes"][key] / row[key]["fused"]["seconds"] / HBM_PEAK_BYTES_PER_S
        for key in ("forward", "forward_backward")}
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pna_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--limit", type=int, default=240, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON row")
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if a.child:
        print(json.dumps(measure(a)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--windows", str(a.windows), "--reps", str(a.reps),
           "--batch", str(a.batch)]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_pna.py: the measurement exceeded {a.limit} s")
    if done.returncode != 0:
        raise SystemExit(f"bench_pna.py: the measurement ended with status {done.returncode}")
    res = {"batch": a.batch, "windows": a.windows, "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "peptides_func": json.loads(done.stdout.decode().strip().splitlines()[-1])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out, "forward_backward": res["peptides_func"]["forward_backward"],
                      "forward": res["peptides_func"]["forward"]}))


if __name__ == "__main__":
    main()
