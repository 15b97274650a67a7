#!/usr/bin/env python3
"""SAN's attention (nn.functional.SANAttentionFn: hscn_san_attn_fwd and the two backward launches, csrc/san.hip) and a
SAN training step on Peptides-func-shaped batches, and beside them, for orientation only, the GPS model with
``local_conv="transformerconv_edge"`` at the same width -- the existing dense per-graph attention and the existing sparse
edge attention in one layer.  Read-only towards the package.  No ratio is promised and there is no pass bar: the two
models compute different things; the numbers are what they are.

Operator: one batch of ``--batch`` graphs, ``--width`` columns in ``--heads`` heads; q, k, v, q2, k2e [N, D] and e [E, D]
are drawn once.  ``full_graph`` on (every ordered pair of a graph) and off (the listed edges alone), forward under
``torch.no_grad()`` and forward + backward with gradients for all six operands.  The pairs a call visits are counted
from the batch (``pairs``: sum of n_g^2; ``edges``), and the arithmetic is 4 C flops per (pair, head) forward (score and
weighted sum): ``flops_over_time`` is that count over the measured time, an achieved rate of the ALGORITHM's flops,
not a share of any peak.

Step: ``SAN`` and ``GPS`` with "atom" / "bond" encoders, ``--layers`` layers, layer norm, no dropout; one step is the
forward, the criterion ("cross_entropy"), the backward and ``zero_grad`` -- no optimizer.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the candidates of a row take turns window by
window, ``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) /
median.  The measurement runs in a child process under a time limit (``--limit`` seconds); the parent never opens the
device.  Writes profiles/san_bench.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]


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
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.loss import criterion
    from graph_hscn.model.gps import GPS
    from graph_hscn.model.san import SAN
    from graph_hscn.nn import functional as Fh
    from graph_hscn.structure import Relation
    from graph_hscn.train import batching
    if not torch.cuda.is_available():
        raise SystemExit("bench_san.py measures on the HIP device: none found")
    dev = "cuda"
    D, heads = a.width, a.heads
    C = D // heads
    graphs = make_dataset("peptides_func", a.batch, seed=0, edge_features=True)
    host = Batch.from_data_list(graphs)
    big = host.to(dev)
    ei = big.edge_index.contiguous()
    N, E, B = int(big.num_nodes), int(ei.size(1)), int(big.num_graphs)
    sizes = (host.ptr[1:] - host.ptr[:-1]).tolist()
    pairs = int(sum(n * n for n in sizes))
    rel = Relation(ei, N, N, both=True)
    g = torch.Generator().manual_seed(0)
    leaves = [torch.randn(r, D, generator=g).to(dev).requires_grad_(True) for r in (N, N, N, E, N, N)]
    q, k, v, e, q2, k2e = leaves
    go = torch.randn(N, D, generator=g).to(dev)

    def op(full):
        def run():
            return Fh.SANAttentionFn.apply(q, k, v, e, q2 if full else None, k2e if full else None, rel, big.ptr32,
                                           int(big.max_nodes), heads, 0.1, full)[0]
        return run

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

    row = {"graphs": B, "nodes": N, "edges": E, "max_nodes": int(big.max_nodes), "pairs": pairs, "width": D,
           "heads": heads, "head_width": C, "gamma": 0.1}
    row["operator_forward"] = windows({"full_graph": fwd(op(True)), "edges_only": fwd(op(False))}, a.windows, a.reps)
    row["operator_forward_backward"] = windows({"full_graph": fwd_bwd(op(True)), "edges_only": fwd_bwd(op(False))},
                                               a.windows, a.reps)
    Fh.check_san(dev)
    # per (pair, head): C multiply-adds for the score and C for the weighted sum (the real score has one more multiply
    # per column); the query-keyed backward pass recomputes the score and adds <g_out, v> and one update (6 C flops),
    # the key-keyed one has two updates (8 C)
    f_flops = 4 * C * heads * pairs
    row["algorithm_flops"] = {"forward": f_flops, "forward_backward": 18 * C * heads * pairs}
    row["flops_over_time"] = {
        "forward": f_flops / row["operator_forward"]["full_graph"]["seconds"],
        "forward_backward": row["algorithm_flops"]["forward_backward"]
        / row["operator_forward_backward"]["full_graph"]["seconds"]}

    relu = ACT_DICT["relu"]
    torch.manual_seed(0)
    models = {"san": SAN(9, D, 10, a.layers, heads, relu, 0.0, "layer", "graph", "atom", "bond", 0.1),
              "san_edges_only": SAN(9, D, 10, a.layers, heads, relu, 0.0, "layer", "graph", "atom", "bond", 0.1,
                                    full_graph=False),
              "gps_transformerconv_edge": GPS(9, D, 10, a.layers, heads, "transformerconv_edge", relu, 0.0, "layer",
                                              "graph", "atom", "bond")}
    steps = {}
    for name, m in models.items():
        m = m.to(dev)
        bd = batching.to_device(m, host, dev)

        def step(m=m, bd=bd):
            m.zero_grad(set_to_none=True)
            loss, _ = criterion("cross_entropy", m(bd), bd.y)
            loss.backward()
        steps[name] = step
    row["step_forward_criterion_backward"] = windows(steps, a.windows, max(1, a.reps // 5))
    for m in models.values():
        m.check_flags()
    row["step_parameters"] = {name: sum(p.numel() for p in m.parameters()) for name, m in models.items()}
    row["layers"] = a.layers
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "san_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON row")
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if a.child:
        print(json.dumps(measure(a)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child"]
    for key in ("windows", "reps", "batch", "width", "heads", "layers"):
        cmd += ["--" + key, str(getattr(a, key))]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_san.py: the measurement exceeded {a.limit} s")
    if done.returncode != 0:
        raise SystemExit(f"bench_san.py: the measurement ended with status {done.returncode}")
    res = {"batch": a.batch, "windows": a.windows, "reps": a.reps,
           "peptides_func": json.loads(done.stdout.decode().strip().splitlines()[-1])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    r = res["peptides_func"]
    print(json.dumps({"written": a.out, "operator_forward": r["operator_forward"],
                      "operator_forward_backward": r["operator_forward_backward"],
                      "step": r["step_forward_criterion_backward"]}))


if __name__ == "__main__":
    main()
