#!/usr/bin/env python3
"""The fused LapPE DeepSet operator (nn.functional.LapPEDeepSetFn: hscn_lappe_fwd, hscn_lappe_bwd, csrc/lappe.hip)
beside the same arithmetic composed from the project's own Linear and torch ops, on the same batch in the same process.
Read-only towards the package.

Shape: one Peptides-func-shaped batch of 128 graphs with the Laplacian statistics of the library's own eigensolver
(transform.compute_posenc_stats_device), K = 10 frequencies, dim_pe = 16, layers = 2, sign flips on under a pinned seed.

Yardstick, taking turns with the operator window by window:
  composed   ``nn.functional.linear`` (csrc/linear.hip, ReLU in the epilogue) twice on the [N K, 2] pairs, a multiply by
             the validity mask and a sum over the K frequencies: what the encoder would be without the operator.  The
             pairs (signs applied, NaN read as 0) and the mask are built ONCE outside the timed region -- the operator
             builds them inside its launch -- so the yardstick is timed for less work than the operator does.
Both run through autograd: forward under ``torch.no_grad()``, forward + backward with gradients for the four parameters.
No ratio is promised; the numbers are what they are.  The one condition the kernel is kept under: the operator's median
for forward + backward is not above the composed one at this shape (``fused_forward_backward_not_above_composed``).

Per call: the medians with their spreads, and the operator's algorithmic bytes computed from the shapes over the measured
time as a share of the HBM peak -- ALGORITHMIC bytes / measured time, not a hardware counter.  The composed path's
[N K, H] intermediates are listed beside them.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the candidates take turns window by window,
``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) / median.
The measurement runs in a child process under a time limit (``--limit`` seconds); the parent never opens the device.
Writes profiles/lappe_bench.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

K, DIM_PE, LAYERS, SEED = 10, 16, 2, 12345
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
    from graph_hscn import _hip
    from graph_hscn.config.config import LapPEConfig
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.nn import functional as Fh
    from graph_hscn.transform.posenc import compute_posenc_stats_device
    if not torch.cuda.is_available():
        raise SystemExit("bench_lappe.py measures on the HIP device: none found")
    dev = "cuda"
    cfg = LapPEConfig(dim_in=9, dim_emb=64, dim_pe=DIM_PE, layers=LAYERS, eigen_max_freqs=K)
    big = Batch.from_data_list(make_dataset("peptides_func", a.batch, seed=0)).to(dev)
    compute_posenc_stats_device(big, True, cfg)
    if int(big.lap_eig_flag.item()) != 0:
        raise SystemExit("bench_lappe.py: the eigensolver flagged the batch")
    vec, val = big.eigvecs_sn.contiguous(), big.eigvals_sn.squeeze(2).contiguous()
    N = int(vec.size(0))
    widths = Fh.lappe_widths(DIM_PE, LAYERS)
    g = torch.Generator().manual_seed(0)
    Ws, bs = [], []
    for i, o in zip(widths[:-1], widths[1:]):
        bound = 1.0 / i ** 0.5
        Ws.append(((torch.rand(o, i, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True))
        bs.append(((torch.rand(o, generator=g) * 2 - 1) * bound).to(dev).requires_grad_(True))
    leaves = Ws + bs
    go = torch.randn(N, DIM_PE, generator=g).to(dev)
    # the composed path's constant inputs, outside the timed region: the signs are the operator's (Philox word 0)
    from tests.lappe_oracle import signs
    sg = signs(K, SEED).to(torch.float32).to(dev)
    mask = (~torch.isnan(vec)).to(torch.float32).unsqueeze(2)
    u = torch.stack((torch.nan_to_num(vec, nan=0.0) * sg, torch.nan_to_num(val, nan=0.0)), 2).view(N * K, 2).contiguous()

    def fused():
        return Fh.LapPEDeepSetFn.apply(vec, val, Ws, bs, SEED)

    def composed():
        h = u
        for W, b in zip(Ws, bs):
            h = Fh.linear(h, W, b, "relu")
        return (h.view(N, K, DIM_PE) * mask).sum(1)

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
        worst = float((fused() - composed()).abs().max())
    if not worst < 1e-4:
        raise SystemExit(f"bench_lappe.py: the operator and the composed ops differ by {worst}")
    fwd_bwd(fused)()
    gf = [t.grad.clone() for t in leaves]
    fwd_bwd(composed)()
    gworst = max(float((a_ - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)) for a_, t in zip(gf, leaves))
    if not gworst < 1e-3:
        raise SystemExit(f"bench_lappe.py: the two backward passes differ by {gworst} of the gradient's size")
    params = sum(t.numel() for t in leaves)
    G = int(_hip.lib().hscn_lappe_workspace_floats(N, K, DIM_PE, LAYERS)) // params
    row = {"graphs": int(big.num_graphs), "nodes": N, "max_freqs": K, "dim_pe": DIM_PE, "layers": LAYERS,
           "samples": N * K, "valid_samples": int(mask.sum().item()), "parameters": params, "backward_workgroups": G,
           "max_abs_difference_to_composed_forward": worst, "max_relative_difference_to_composed_gradients": gworst}
    row["forward"] = windows({"fused": fwd(fused), "composed": fwd(composed)}, a.windows, a.reps)
    row["forward_backward"] = windows({"fused": fwd_bwd(fused), "composed": fwd_bwd(composed)}, a.windows, a.reps)
    for key in ("forward", "forward_backward"):
        ours, ya = row[key]["fused"], row[key]["composed"]
        row[key]["fused_over_composed"] = ours["seconds"] / ya["seconds"]
        row[key]["ratio_beyond_composed_spread"] = bool(abs(ours["seconds"] - ya["seconds"]) > ya["spread"] * ya["seconds"])
    row["fused_forward_backward_not_above_composed"] = bool(
        row["forward_backward"]["fused"]["seconds"] <= row["forward_backward"]["composed"]["seconds"])
    # forward: vec, val in, the parameters per workgroup through the caches once, out; backward: vec, val, g_out in, the
    # per-workgroup partials out and in again, the gradients out
    f_bytes = 4 * (2 * N * K + params + N * DIM_PE)
    b_bytes = 4 * (2 * N * K + N * DIM_PE + params + 2 * G * params + params)
    row["algorithmic_bytes"] = {"forward": f_bytes, "backward": b_bytes, "forward_backward": f_bytes + b_bytes}
    row["composed_intermediate_bytes"] = {f"[N K, {w}]": 4 * N * K * w for w in widths[1:]}
    row["algorithmic_bytes_over_time_share_of_hbm_peak"] = {
        key: row["algorithmic_bytes"][key] / row[key]["fused"]["seconds"] / HBM_PEAK_BYTES_PER_S
        for key in ("forward", "forward_backward")}
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lappe_bench.json"))
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
        raise SystemExit(f"bench_lappe.py: the measurement exceeded {a.limit} s")
    if done.returncode != 0:
        raise SystemExit(f"bench_lappe.py: the measurement ended with status {done.returncode}")
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
