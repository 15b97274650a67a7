#!/usr/bin/env python3
"""The MPNN baseline with conv_type "gat": the narrow-row self-loop GAT kernels (csrc/gat_loops.hip) beside the
wave-per-row kernels (csrc/gat.hip) over the explicit-loop relation on the SAME inputs, the dispatch threshold between
them, and the whole layered training step beside the GCN baseline's.  Read-only towards the package.

Timing: HIP events around ``reps`` re-issues of one call, after a warm-up; ``regions`` such regions per number, the
median reported with the spread (max - min) / median.  Bytes are algorithmic (every array the call must touch, once),
reported over the median time as a fraction of the 8 TB/s HBM peak.  Writes profiles/r05_gat_mpnn.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

from graph_hscn._hip import call, ptr, stream
from graph_hscn.config.config import MPNNConfig
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.mpnn import build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import Relation, with_self_loops

HBM_PEAK = 8.0e12
DEV = "cuda"


def timed(fn, reps, regions, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    med = statistics.median(us)
    return {"us": med, "spread": (max(us) - min(us)) / med}


class Case:
    """One edge list, width and set of inputs; the six launches as closures."""

    def __init__(self, ei, n, width, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.n, self.w = n, width
        self.raw = Relation(ei, n, n, both=True)
        self.loops = Relation(with_self_loops(ei, n), n, n, both=True)
        self.loops.pos_t
        f = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
        self.h, self.g = f(n, width), f(n, width)
        self.a_s, self.a_d = f(n), f(n)
        self.att_s, self.att_d, self.bias = f(width), f(width), f(width)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
        self.out, self.g_h = z(n, width), z(n, width)
        self.stat, self.tsum, self.g_a = z(n, 2), z(n), z(n, 2)
        El = self.loops.num_edges
        self.alpha, self.g_pre = z(El), z(El)
        self.g_a_s, self.g_a_d = z(n), z(n)
        self.E, self.El = self.raw.num_edges, El

    def narrow(self):
        r, s = self.raw, self
        return {
            "fwd": lambda: call("hscn_gat_loop_fwd", ptr(r.csr.rowptr), ptr(r.csr.col), ptr(s.a_s), ptr(s.a_d), ptr(s.h),
                                ptr(s.bias), ptr(s.stat), ptr(s.out), s.n, s.w, 0.2, 1, stream()),
            "bwd_dst": lambda: call("hscn_gat_loop_bwd_dst", ptr(r.csr.rowptr), ptr(r.csr.col), ptr(s.a_s), ptr(s.a_d),
                                    ptr(s.h), ptr(s.stat), ptr(s.g), ptr(s.tsum), ptr(s.g_a), s.n, s.w, 0.2, stream()),
            "bwd_src": lambda: call("hscn_gat_loop_bwd_src", ptr(r.csr_t.rowptr), ptr(r.csr_t.col), ptr(s.a_s),
                                    ptr(s.a_d), ptr(s.h), ptr(s.stat), ptr(s.tsum), ptr(s.g), ptr(s.att_s), ptr(s.att_d),
                                    ptr(s.g_a), ptr(s.g_h), s.n, s.w, 0.2, stream()),
        }

    def wide(self):
        r, s = self.loops, self
        return {
            "fwd": lambda: call("hscn_gat_segment_fwd", ptr(r.csr.rowptr), ptr(r.csr.col), ptr(s.a_s), ptr(s.a_d),
                                ptr(s.h), ptr(s.bias), ptr(s.alpha), ptr(s.out), s.n, s.w, 0.2, 0, 1, stream()),
            "bwd_dst": lambda: call("hscn_gat_segment_bwd_dst", ptr(r.csr.rowptr), ptr(r.csr.col), ptr(s.a_s),
                                    ptr(s.a_d), ptr(s.h), ptr(s.alpha), ptr(s.g), ptr(s.g_pre), ptr(s.g_a_d), s.n, s.w,
                                    0.2, stream()),
            "bwd_src": lambda: call("hscn_gat_segment_bwd_src", ptr(r.csr_t.rowptr), ptr(r.csr_t.col), ptr(r.pos_t),
                                    ptr(s.alpha), ptr(s.g_pre), ptr(s.g), ptr(s.att_s), ptr(s.g_a_s), ptr(s.g_h), s.n,
                                    s.w, stream()),
        }

    def bytes(self):
        """Algorithmic bytes per launch: index arrays, per-node scalars, feature rows and per-edge arrays, each once."""
        n, w, E, El = self.n, self.w, self.E, self.El
        row = 4 * n * w
        return {
            "narrow": {"fwd": 4 * (n + 1) + 4 * E + 8 * n + row + 4 * w + 8 * n + row,
                       "bwd_dst": 4 * (n + 1) + 4 * E + 8 * n + 2 * row + 8 * n + 8 * n,
                       "bwd_src": 4 * (n + 1) + 4 * E + 8 * n + 2 * row + 8 * n + 4 * n + 8 * w + 8 * n + row},
            "wide": {"fwd": 4 * (n + 1) + 4 * El + 8 * n + row + 4 * w + 4 * El + row,
                     "bwd_dst": 4 * (n + 1) + 4 * El + 8 * n + 2 * row + 4 * El + 4 * El + 4 * n,
                     "bwd_src": 4 * (n + 1) + 8 * El + 8 * El + row + 4 * w + 4 * n + row},
        }


def kernel_rows(ei, n, width, reps, regions):
    c = Case(ei, n, width)
    nb = c.bytes()
    out = {"nodes": n, "edges": c.E, "edges_with_loops": c.El, "max_in_degree": c.raw.max_in_degree}
    for _ in range(3):                      # the forward's hand-over buffers hold real values for the backward timings
        for k in ("fwd", "bwd_dst", "bwd_src"):
            c.narrow()[k]()
            c.wide()[k]()
    for k in ("fwd", "bwd_dst", "bwd_src"):
        for side, fns in (("narrow", c.narrow()), ("wide", c.wide())):
            t = timed(fns[k], reps, regions)
            t["bytes"] = nb[side][k]
            t["hbm_fraction"] = nb[side][k] / (t["us"] * 1e-6) / HBM_PEAK
            out[f"{k}_{side}"] = t
    return out


def with_hub(ei, n, degree):
    """``ei`` plus edges that raise node 0 to ``degree`` more in-edges from distinct sources."""
    src = 1 + torch.arange(degree, dtype=torch.int64, device=ei.device) % (n - 1)
    return torch.cat([ei, torch.stack([src, torch.zeros_like(src)])], 1).contiguous()


def threshold_rows(ei, n, width, reps, regions):
    rows = []
    for d in (4, 8, 16, 32, 64, 128, 256, 1024):
        c = Case(with_hub(ei, n, d), n, width)
        row = {"max_in_degree": c.raw.max_in_degree}
        for side, fns in (("narrow", c.narrow()), ("wide", c.wide())):
            def all_three(fns=fns):
                fns["fwd"]()
                fns["bwd_dst"]()
                fns["bwd_src"]()
            row[side] = timed(all_three, reps, regions)
        rows.append(row)
    return rows


def step_rows(batch, B, K, regions):
    out = {}
    y = (torch.rand(B, 10, generator=torch.Generator().manual_seed(0)) < 0.2).float().to(DEV)
    for conv in ("gat", "gcn"):
        torch.manual_seed(0)
        m = build_mpnn(MPNNConfig(conv, "relu"), 9, 10).to(DEV).train()

        def step():
            for p in m.parameters():
                p.grad = None
            loss, _ = criterion("cross_entropy", m(batch), y)
            loss.backward()

        row = {"eager": timed(step, K, regions, warmup=10)}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        row["captured"] = timed(g.replay, K, regions, warmup=5)
        out[conv] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_gat_mpnn.json"))
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gat_mpnn.py measures on the HIP device: none found")
    B = a.batch
    b = Batch.from_data_list(make_dataset("peptides_func", B, seed=0)).to(DEV)
    b.x = b.x.float()
    n = int(b.x.shape[0])
    ei = b.edge_index.contiguous()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "reps": a.reps, "regions": a.regions,
           "hbm_peak_bytes_per_s": HBM_PEAK, "dispatch_threshold": int(Fh.GAT_NARROW_MAX_DEGREE), "kernels": {}}
    for w in (16, 10):
        res["kernels"][f"width_{w}"] = kernel_rows(ei, n, w, a.reps, a.regions)
        print(f"width {w}", json.dumps(res["kernels"][f"width_{w}"]), file=sys.stderr, flush=True)
    res["threshold_sweep_width_16"] = threshold_rows(ei, n, 16, max(a.reps // 4, 10), a.regions)
    print("sweep", json.dumps(res["threshold_sweep_width_16"]), file=sys.stderr, flush=True)
    res["training_step"] = step_rows(b, B, max(a.reps // 4, 10), a.regions)
    print("step", json.dumps(res["training_step"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
