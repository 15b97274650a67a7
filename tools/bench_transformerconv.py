#!/usr/bin/env python3
"""TransformerConv's launches (hscn_edge_attn_fwd, hscn_edge_attn_bwd_dst + hscn_edge_attn_bwd_src,
csrc/edge_attention.hip) beside the GAT segment operator's (hscn_gat_segment_fwd, hscn_gat_segment_bwd_dst +
hscn_gat_segment_bwd_src, csrc/gat.hip; one head of the same total width) on the same relation in the same process.
Read-only towards the package.

Shapes, all at total width 64, from one Peptides-func-shaped batch of 128 graphs:

  ll-h1 / ll-h4 / ll-h8   the local -> local relation (in-degree 2..4) with 1, 4 and 8 heads
  lv-K4 / lv-K64          the local -> virtual relation of the same batch with K = 4 and K = 64 clusters per graph
                          (every node points at one cluster of its graph, drawn uniformly), 4 heads

The yardstick is GAT's segment operator in the same run.  It is not the same arithmetic: GAT reads one logit pair and
one H-wide source row per edge and keeps an [E] tensor of weights; the attention reads three Hd*C-wide rows per edge and
keeps one log-sum-exp pair per (node, head).  No ratio is promised; the table is what it is.

Per shape: forward and forward + backward of both, the ratio with the spread of either timing, and the algorithmic
bytes of the attention's launches computed from the shapes over the kernel time as a share of the HBM peak --
ALGORITHMIC bytes / measured time, not a hardware counter; rows gathered through the caches count once per edge, so a
share above what the memory system delivers says that the gathers hit in cache.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; the two operators take turns window by
window, ``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) /
median.  Every shape is measured by a child process of its own under a time limit (``--limit`` seconds); the parent
never opens the device, and a child that fails or runs out of time ends the run: nothing is started after it.  Writes
profiles/transformerconv_bench.json (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

WIDTH = 64
CASES = {"ll-h1": ("ll", 1, None), "ll-h4": ("ll", 4, None), "ll-h8": ("ll", 8, None),
         "lv-K4": ("lv", 4, 4), "lv-K64": ("lv", 4, 64)}
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


def algorithmic_bytes(Nd, Ns, E, heads, HC, edge_features=False):
    """What the three launches must move, from the shapes alone (float32 and int32 are 4 bytes): per edge the k and v
    rows (and e), col and eid; per target q, out, the log-sum-exp pair; the backward reads them again with the cotangent
    and writes dq / de, delta, then per edge q and the cotangent rows, per source k, v, dk, dv."""
    e = E * HC if edge_features else 0
    fwd = 4 * ((Nd + 1) + 2 * E + Nd * HC + 2 * E * HC + e + Nd * HC + 2 * Nd * heads)
    dst = 4 * ((Nd + 1) + 2 * E + 3 * Nd * HC + 2 * E * HC + e + 2 * Nd * heads + Nd * heads + Nd * HC + e)
    src = 4 * ((Ns + 1) + 2 * E + 2 * Ns * HC + 2 * E * HC + e + 3 * E * heads + 2 * Ns * HC)
    return {"forward": fwd, "backward": dst + src, "forward_backward": fwd + dst + src}


def measure(name, a):
    import numpy as np
    import torch
    from graph_hscn import _hip
    from graph_hscn._hip import ptr, stream
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.structure import Relation
    if not torch.cuda.is_available():
        raise SystemExit("bench_transformerconv.py measures on the HIP device: none found")
    dev = "cuda"
    kind, heads, K = CASES[name]
    big = Batch.from_data_list(make_dataset("peptides_func", a.batch, seed=0))
    N = int(big.num_nodes)
    if kind == "ll":
        ei, Ns, Nd = big.edge_index.to(dev), N, N
    else:
        rng = np.random.default_rng(0)
        cluster = torch.from_numpy(rng.integers(0, K, N)) + big.batch * K
        ei, Ns, Nd = torch.stack([torch.arange(N), cluster]).to(dev), N, a.batch * K
    E = int(ei.size(1))
    rel = Relation(ei.contiguous(), Ns, Nd, both=True)
    c, t = rel.csr, rel.csr_t
    pos_t = rel.pos_t
    HC, C = WIDTH, WIDTH // heads
    g = torch.Generator().manual_seed(heads)
    rand = lambda *s: torch.randn(*s, generator=g).to(dev)                 # noqa: E731
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    q, k, v, go = rand(Nd, HC), rand(Ns, HC), rand(Ns, HC), rand(Nd, HC)
    out, lse, delta, dq, dk, dv = new(Nd, HC), new(Nd, heads, 2), new(Nd, heads), new(Nd, HC), new(Ns, HC), new(Ns, HC)
    # the GAT segment operator's tensors: one head of width HC
    hs, a_s, a_d = rand(Ns, HC), rand(Ns), rand(Nd)
    att_s = rand(HC)
    alpha, g_out, g_pre, g_a_d, g_a_s, g_hs = new(max(E, 1)), new(Nd, HC), new(max(E, 1)), new(Nd), new(Ns), new(Ns, HC)
    st = stream()

    def attn_fwd():
        _hip.call("hscn_edge_attn_fwd", ptr(c.rowptr), ptr(c.col), ptr(c.eid), ptr(q), ptr(k), ptr(v), None, ptr(out),
                  ptr(lse), Nd, Ns, E, heads, C, ptr(c.flag), st)

    def attn_bwd():
        _hip.call("hscn_edge_attn_bwd_dst", ptr(c.rowptr), ptr(c.col), ptr(c.eid), ptr(q), ptr(k), ptr(v), None,
                  ptr(out), ptr(lse), ptr(go), ptr(delta), ptr(dq), None, Nd, Ns, E, heads, C, ptr(c.flag), st)
        _hip.call("hscn_edge_attn_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(t.eid), ptr(q), ptr(k), ptr(v), None,
                  ptr(lse), ptr(delta), ptr(go), ptr(dk), ptr(dv), Nd, Ns, E, heads, C, ptr(c.flag), st)

    def gat_fwd():
        _hip.call("hscn_gat_segment_fwd", ptr(c.rowptr), ptr(c.col), ptr(a_s), ptr(a_d), ptr(hs), None, ptr(alpha),
                  ptr(g_out), Nd, HC, 0.2, 0, 0, st)

    def gat_bwd():
        _hip.call("hscn_gat_segment_bwd_dst", ptr(c.rowptr), ptr(c.col), ptr(a_s), ptr(a_d), ptr(hs), ptr(alpha),
                  ptr(go), ptr(g_pre), ptr(g_a_d), Nd, HC, 0.2, st)
        _hip.call("hscn_gat_segment_bwd_src", ptr(t.rowptr), ptr(t.col), ptr(pos_t), ptr(alpha), ptr(g_pre), ptr(go),
                  ptr(att_s), ptr(g_a_s), ptr(g_hs), Ns, HC, st)

    def both(f, b):
        return lambda: (f(), b())

    deg = (c.rowptr[1:] - c.rowptr[:-1])
    row = {"shape": name, "relation": kind, "graphs": a.batch, "heads": heads, "head_dim": C, "width": HC, "K": K,
           "sources": Ns, "targets": Nd, "edges": E, "largest_in_degree": int(deg.max()),
           "mean_in_degree": float(deg.float().mean())}
    row["forward"] = windows({"attention": attn_fwd, "gat": gat_fwd}, a.windows, a.reps)
    row["forward_backward"] = windows({"attention": both(attn_fwd, attn_bwd), "gat": both(gat_fwd, gat_bwd)},
                                      a.windows, a.reps)
    torch.cuda.synchronize()
    if not all(bool(torch.isfinite(x).all()) for x in (out, dq, dk, dv, g_out, g_hs)) or int(c.flag.item()) != 0:
        raise SystemExit("bench_transformerconv.py: a non-finite result or a flagged slot")
    for key in ("forward", "forward_backward"):
        at, ga = row[key]["attention"], row[key]["gat"]
        row[key]["attention_over_gat"] = at["seconds"] / ga["seconds"]
        # the run-to-run spread of the yardstick's timing itself is the yardstick for the ratio
        row[key]["ratio_beyond_gat_spread"] = bool(abs(at["seconds"] - ga["seconds"]) > ga["spread"] * ga["seconds"])
    nbytes = algorithmic_bytes(Nd, Ns, E, heads, HC)
    row["algorithmic_bytes"] = nbytes
    row["algorithmic_bytes_over_time_share_of_hbm_peak"] = {
        key: nbytes[key] / row[key]["attention"]["seconds"] / HBM_PEAK_BYTES_PER_S for key in ("forward", "forward_backward")}
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformerconv_bench.json"))
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
    res = {"batch": a.batch, "windows": a.windows, "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
           "shapes": {}}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--windows", str(a.windows), "--reps",
               str(a.reps), "--batch", str(a.batch)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_transformerconv.py: {name} exceeded {a.limit} s; nothing further was started")
        if done.returncode != 0:
            raise SystemExit(f"bench_transformerconv.py: {name} ended with status {done.returncode}; nothing further "
                             "was started")
        res["shapes"][name] = json.loads(done.stdout.decode().strip().splitlines()[-1])
        print(json.dumps({name: res["shapes"][name]}), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
