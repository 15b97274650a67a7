#!/usr/bin/env python3
"""BASELINE config 1 (the MPNN GCN baseline, configs/GCN/peptides_func_GCN.yaml: hidden 16, 3 layers,
dropout 0.2, batch 32) -- forward + criterion + backward per step on the HIP path, beside the CPU oracle
on this box's host cores.  A parity-case measurement, not the bench line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import torch

import bench
from graph_hscn.config.config import MPNNConfig
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.loss import criterion
from graph_hscn.model.mpnn import build_mpnn
from graph_hscn.step import MPNNResidentTrainStep
from oracle import models as OM


def epoch_rows(B, iters=20):
    """Whole epochs on the device (train_resident.fit_resident's loop): one replay = gather of the next permutation
    slice + the one-launch step + AdamW (optim.FlatAdam), over a DeviceGraphDataset of 20 B graphs; and fit_resident
    itself (3 epochs, with its eager tail batch and evaluation), per iteration of wall time."""
    from graph_hscn.config.config import OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.loader.device_dataset import DeviceGraphDataset
    from graph_hscn.optim import FlatAdam
    from graph_hscn.replay import CapturedStep
    from graph_hscn.train.train_resident import fit_resident
    graphs = make_dataset("peptides_func", iters * B + 3, seed=1)
    torch.manual_seed(0)
    m = build_mpnn(MPNNConfig("gcn", "relu"), 9, 10).to("cuda").train()
    ds = DeviceGraphDataset(graphs[: iters * B], "cuda", B)
    ds.new_epoch(torch.Generator(device="cuda").manual_seed(0))
    opt = lambda st: FlatAdam.from_config("adamW", st.param_grads, st.grads, lr=1e-3, weight_decay=0.0)  # noqa: E731
    cs = CapturedStep(m, ds.static, "cross_entropy", optimizer=opt, pre=ds.gather_next)
    ds.new_epoch()
    for _ in range(iters):
        cs.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        ds.new_epoch()
        t0 = time.perf_counter()
        for _ in range(iters):
            cs.replay()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters)
    ds.check()
    m2 = build_mpnn(MPNNConfig("gcn", "relu"), 9, 10).to("cuda")
    tc = TrainingConfig("mpnn", "cross_entropy", "ap", epochs=3, eval_period=100, patience=100)
    ev = [DataLoader(graphs[-3:], batch_size=3)] * 2
    train = graphs[: iters * B + 1]                     # one graph of eager tail per epoch
    fit_resident(None, OptimConfig("adamW", lr=1e-3), tc, train, ev, m2, batch_size=B)   # (warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit_resident(None, OptimConfig("adamW", lr=1e-3), tc, train, ev, m2, batch_size=B)
    torch.cuda.synchronize()
    fit = (time.perf_counter() - t0) / (3 * (iters + 1))
    return {"device_epoch_iter_us": best * 1e6, "device_epoch_graphs_per_s": B / best,
            "fit_resident_wall_us_per_iter": fit * 1e6}


def main():
    out = {}
    for B in (1, 32, 128, 1024):
        b = Batch.from_data_list(make_dataset("peptides_func", B, seed=0))
        y = (torch.rand(B, 10, generator=torch.Generator().manual_seed(0)) < 0.2).float()
        d = b.to("cuda")
        d.x = d.x.float()
        yd = y.to("cuda")
        torch.manual_seed(0)
        m = build_mpnn(MPNNConfig("gcn", "relu"), 9, 10).to("cuda").train()

        def step():
            for p in m.parameters():
                p.grad = None
            loss, _ = criterion("cross_entropy", m(d), yd)
            loss.backward()

        for _ in range(10):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        K = 100
        for _ in range(K):
            step()
        torch.cuda.synchronize()
        eager = (time.perf_counter() - t0) / K
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            g.replay()
        torch.cuda.synchronize()
        rep = (time.perf_counter() - t0) / K
        row = {"eager_ms": eager * 1e3, "replay_ms": rep * 1e3, "replay_graphs_per_s": B / rep}
        # the same step as ONE launch + the gradient fold (step.MPNNResidentTrainStep), replayed from a hipGraph
        d.y = yd
        rs = MPNNResidentTrainStep(m, d, "cross_entropy")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                rs.run()
        torch.cuda.current_stream().wait_stream(s)
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            rs.run()
        for _ in range(5):
            g1.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            g1.replay()
        torch.cuda.synchronize()
        rrep = (time.perf_counter() - t0) / K
        rs.check()
        row.update(resident_replay_us=rrep * 1e6, resident_graphs_per_s=B / rrep)
        if B <= 128:
            nt = min(4, bench.host_cores())      # tiny ops: a few intra-op threads beat all cores (bench.py sweep)
            torch.set_num_threads(nt)
            om = OM.MPNN(OM.ACT["relu"], 9, 16, 10, 3, 0.2).train()
            x = b.x.float()

            def cstep():
                om.zero_grad(set_to_none=True)
                loss, _ = OM.criterion("cross_entropy", om(x, b.edge_index, b.batch, B), y)
                loss.backward()

            for _ in range(3):
                cstep()
            t0 = time.perf_counter()
            for _ in range(20):
                cstep()
            c = (time.perf_counter() - t0) / 20
            row.update(cpu_oracle_ms=c * 1e3, cpu_graphs_per_s=B / c, cpu_threads=nt)
        if B in (32, 128):
            row.update(epoch_rows(B))
        out[f"B={B}"] = row
        print(f"B={B}", row, file=sys.stderr, flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
