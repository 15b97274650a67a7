#!/usr/bin/env python3
"""GCN2Conv as ONE launch (nn.functional.GCN2ConvFn: hscn_gcn2_fwd; backward hscn_gcn2_bwd, hscn_gcn2_bwd_w and the
gather) against the same layer COMPOSED from the operators the package had before it -- ``spmm_gcn_raw`` for A_hat x, a
torch elementwise mix with x0, ``linear_raw`` (in column chunks where the weight exceeds its LDS image, as
``linear_wide`` cuts it), a torch elementwise blend and ``hscn_act_fwd``; backward ``act_bwd_raw``, ``linear_raw`` with the
transposed layout, ``linear_bwd_w_raw`` and the gather.  The composed layer is written here and never used by the
package.  Read-only towards the package; reads nothing outside the repository.  No ratio is promised and there is no
pass bar: the numbers are what they are.

Shapes: a Peptides-func-shaped batch (``--batch`` graphs of loader.synthetic) and a PascalVOC-SP-sized one (``--voc``
graphs of 479 nodes and 2710 directed edges each, drawn here), at H in {64, 128, 300}; alpha = 0.1, beta = log(0.5 / 8
+ 1), ReLU, shared weights.  Operator forward under ``torch.no_grad()``; forward + backward with gradients for x, x0 and
the weight.  Step: ``GCNII`` with 16 layers, a Linear node encoder, no dropout: forward, criterion ("cross_entropy"),
backward, ``zero_grad`` -- no optimizer; once with the fused layer and once with the composed layer put in its place.

Launch counts per layer: the ``hscn_*`` calls are counted through ``_hip.call``, the torch elementwise kernels of the
composed layer by hand where they are issued.

Timing: device events around ``--reps`` back-to-back calls, after a warm-up; fused and composed take turns window by
window, ``--windows`` windows per number (default 9, at least 7); the median per call with the spread (max - min) /
median.  The measurement runs in a child process under a time limit (``--limit`` seconds); the parent never opens the
device.  Writes profiles/gcn2_bench.json (--out)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

WIDTHS = (64, 128, 300)
ALPHA, BETA = 0.1, math.log(0.5 / 8 + 1.0)


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


def composed_layer():
    """The layer out of the earlier operators, as an autograd Function with GCN2ConvFn's signature (shared weights)."""
    import torch
    from graph_hscn.nn import functional as Fh
    torch_kernels = {"forward": 0, "backward": 0}

    def chunks(W):                                     # column chunks of a [I, O] weight that fit linear's LDS image
        I, O = W.shape
        step = O if I * O * 4 <= Fh.LINEAR_MAX_WEIGHT_BYTES else (Fh.LINEAR_MAX_WEIGHT_BYTES // (4 * I)) // 4 * 4
        return [W[:, o:o + step].contiguous() for o in range(0, O, step)]

    def times(x, parts, layout):
        ys = [Fh.linear_raw(x, w, w_layout=layout)[0] for w in parts]
        return ys[0] if len(ys) == 1 else torch.cat(ys, 1)

    class Composed(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, x0, W1, W2, rel, alpha, beta, act):
            p = Fh.spmm_gcn_raw(rel.csr, rel.dinv, rel.dinv, x)
            h = torch.add(p.mul_(1.0 - alpha), x0, alpha=alpha)                    # 2 elementwise kernels
            hw = times(h, chunks(W1), 1)
            y = torch.add(hw.mul_(beta), h, alpha=1.0 - beta)                      # 2
            wide = W1.shape[0] * W1.shape[1] * 4 > Fh.LINEAR_MAX_WEIGHT_BYTES
            torch_kernels["forward"] = 4 + (1 if wide else 0)                      # + the cat of the column chunks
            out = torch.empty_like(y)
            Fh.call("hscn_act_fwd", Fh.ptr(y), Fh.ptr(out), y.numel(), act, Fh.stream())
            ctx.rel, ctx.alpha, ctx.beta, ctx.act = rel, alpha, beta, act
            ctx.save_for_backward(W1, out, h)
            return out

        @staticmethod
        def backward(ctx, g):
            W1, out, h = ctx.saved_tensors
            gy = Fh.act_bwd_raw(g.contiguous(), out, ctx.act)
            wide = W1.shape[0] * W1.shape[1] * 4 > Fh.LINEAR_MAX_WEIGHT_BYTES
            rows = chunks(W1.t().contiguous()) if wide else [W1]                   # gy W1^T: layout 0 reads W1 as it is
            ghw = times(gy, rows, 1 if wide else 0)
            gh = torch.add(ghw.mul_(ctx.beta), gy, alpha=1.0 - ctx.beta)           # 2
            gW = Fh.linear_bwd_w_raw(h, gy, True, False)[0].mul_(ctx.beta)         # 1
            gx0 = gh * ctx.alpha                                                   # 1
            gp = gh.mul_(1.0 - ctx.alpha)                                          # 1
            torch_kernels["backward"] = 5 + (2 if wide else 0)                     # + the transpose and the cat
            gx = Fh.spmm_gcn_raw(ctx.rel.csr_t, ctx.rel.dinv, ctx.rel.dinv, gp)
            return gx, gx0, gW, None, None, None, None, None

    return Composed, torch_kernels


class CallCount:
    def __init__(self):
        from graph_hscn import _hip
        from graph_hscn.nn import functional as Fh
        self.names, self._mods, self._real = [], (_hip, Fh), _hip.call

    def __enter__(self):
        def call(name, *a):
            self.names.append(name)
            return self._real(name, *a)
        for m in self._mods:
            m.call = call
        return self

    def __exit__(self, *exc):
        for m in self._mods:
            m.call = self._real


def voc_batch(count, seed=0):
    """``count`` graphs of PascalVOC-SP's mean size: 479 nodes, 1355 undirected pairs = 2710 directed edges."""
    import torch
    from graph_hscn.data import Batch, Data
    g = torch.Generator().manual_seed(seed)
    graphs = []
    for _ in range(count):
        half = torch.randint(0, 479, (2, 1355), generator=g)
        graphs.append(Data(x=torch.randn(479, 14, generator=g), edge_index=torch.cat([half, half.flip(0)], 1),
                           y=torch.zeros(1, 10)))
    return Batch.from_data_list(graphs)


def measure(a):
    import torch
    from graph_hscn._hip import ACT
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import Batch
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.loss import criterion
    from graph_hscn.model.gcnii import GCNII
    from graph_hscn.nn import functional as Fh
    from graph_hscn.structure import self_loop_relation_of
    from graph_hscn.train import batching
    if not torch.cuda.is_available():
        raise SystemExit("bench_gcn2.py measures on the HIP device: none found")
    dev = "cuda"
    Composed, torch_kernels = composed_layer()
    fused = Fh.GCN2ConvFn
    shapes = {"peptides_func": Batch.from_data_list(make_dataset("peptides_func", a.batch, seed=0)),
              "pascalvoc_sp_sized": voc_batch(a.voc)}
    res = {}
    for shape, host in shapes.items():
        ei = host.edge_index.to(dev).contiguous()
        N, E = int(host.num_nodes), int(ei.size(1))
        rel = self_loop_relation_of(ei, N, both=True)
        rel.dinv
        rows = {}
        for H in WIDTHS:
            g = torch.Generator().manual_seed(H)
            x, x0 = (torch.randn(N, H, generator=g).to(dev).requires_grad_(True) for _ in range(2))
            W = (torch.randn(H, H, generator=g) / math.sqrt(H)).to(dev).requires_grad_(True)
            go = torch.randn(N, H, generator=g).to(dev)
            leaves = (x, x0, W)

            def op(fn):
                return lambda: fn.apply(x, x0, W, None, rel, ALPHA, BETA, ACT["relu"])

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

            row = {"plan": Fh.gcn2_plan(H)}
            calls = {}
            for name, fn in (("fused", fused), ("composed", Composed)):
                with CallCount() as c:
                    out = op(fn)()
                    nf = list(c.names)
                    del c.names[:]
                    out.backward(go)
                    nb = list(c.names)
                tk = torch_kernels if name == "composed" else {"forward": 0, "backward": 0}
                calls[name] = {"forward_hscn_calls": nf, "backward_hscn_calls": nb,
                               "forward_torch_kernels": tk["forward"], "backward_torch_kernels": tk["backward"]}
            a_out, b_out = op(fused)().detach(), op(Composed)().detach()
            row["max_abs_difference_fused_composed"] = float((a_out - b_out).abs().max())
            row["launches"] = calls
            row["operator_forward"] = windows({"fused": fwd(op(fused)), "composed": fwd(op(Composed))}, a.windows, a.reps)
            row["operator_forward_backward"] = windows({"fused": fwd_bwd(op(fused)), "composed": fwd_bwd(op(Composed))},
                                                       a.windows, max(1, a.reps // 2))
            torch.manual_seed(0)
            m = GCNII(int(host.x.size(1)), H, 10, a.layers, ACT_DICT["relu"], 0.0).to(dev)
            bd = batching.to_device(m, host, dev)
            target = (torch.rand(int(host.num_graphs), 10, generator=g) < 0.3).float().to(dev)

            def step(fn):
                def run():
                    Fh.GCN2ConvFn = fn                # the layer module looks the Function up at call time
                    try:
                        m.zero_grad(set_to_none=True)
                        loss, _ = criterion("cross_entropy", m(bd), target)
                        loss.backward()
                    finally:
                        Fh.GCN2ConvFn = fused
                return run
            row["step_forward_criterion_backward"] = windows({"fused": step(fused), "composed": step(Composed)},
                                                             a.windows, max(1, a.reps // 10))
            for part in ("operator_forward", "operator_forward_backward", "step_forward_criterion_backward"):
                row[part]["fused_over_composed"] = row[part]["fused"]["seconds"] / row[part]["composed"]["seconds"]
            rows[str(H)] = row
            del x, x0, W, go, m, bd
            torch.cuda.empty_cache()
        res[shape] = {"graphs": int(host.num_graphs), "nodes": N, "edges": E, "widths": rows}
    res["layers"] = a.layers
    res["alpha"], res["beta"] = ALPHA, BETA
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gcn2_bench.json"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--voc", type=int, default=32)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--limit", type=int, default=400, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON result")
    a = ap.parse_args()
    if a.windows < 7:
        raise SystemExit("at least 7 windows per number")
    if a.child:
        print(json.dumps(measure(a)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child"]
    for key in ("windows", "reps", "batch", "voc", "layers"):
        cmd += ["--" + key, str(getattr(a, key))]
    try:
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"bench_gcn2.py: the measurement exceeded {a.limit} s")
    if done.returncode != 0:
        raise SystemExit(f"bench_gcn2.py: the measurement ended with status {done.returncode}")
    res = {"windows": a.windows, "reps": a.reps}
    res.update(json.loads(done.stdout.decode().strip().splitlines()[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for shape in ("peptides_func", "pascalvoc_sp_sized"):
        for H, row in res[shape]["widths"].items():
            brief[f"{shape} H={H}"] = {part: [round(row[part][k]["seconds"] * 1e6, 1) for k in ("fused", "composed")]
                                       for part in ("operator_forward", "operator_forward_backward",
                                                    "step_forward_criterion_backward")}
    print(json.dumps({"written": a.out, "microseconds_fused_composed": brief}))


if __name__ == "__main__":
    main()
