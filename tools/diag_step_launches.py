#!/usr/bin/env python3
"""Phase stamps of the one-launch training step over N launches of one process (diagnostic build only).

  make -C graph-hscn_amd diag && HSCN_LIB=graph-hscn_amd/graph_hscn/lib/libhscn_diag.so python tools/diag_step_launches.py N [uniform]

tools/diag_step.py reads one launch, and a phase of one workgroup moves by several hundred cycles from launch to
launch.  This prints, for the two workgroups of the benchmark batch's largest graph and for the slowest workgroups, the
median (min - max) over N launches of the phases that the front of the step decides."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import numpy as np
import torch

import bench
from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT
from graph_hscn.model.hscn import HSCN
from graph_hscn.step import ResidentTrainStep


def main():
    N = int(sys.argv[1])
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    ids = "uniform" if "uniform" in sys.argv[2:] else "scn_untrained"
    shape, B0, K0, C0, loss0 = bench.WORKLOADS["peptides_func"]
    hb_host, graphs, _ = bench.build_hetero_batch(shape, B0, K0, 0, dev, ids)
    hb = hb_host.to(dev)
    torch.manual_seed(0)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], hb_host["local"].x.size(1), 16, C0, 3).to(dev)
    B = hb.num_graphs
    buf = torch.zeros(2 * B, 64, dtype=torch.int64, device=dev)
    lib.hscn_diag_set_stamp_buffer.argtypes = [ctypes.c_void_p]
    assert lib.hscn_diag_set_stamp_buffer(buf.data_ptr()) == 0
    sizes = np.diff(hb_host["local"].ptr.numpy())
    g = int(np.argmax(sizes))
    rs = ResidentTrainStep(model, hb, loss0, one_launch=True)
    for _ in range(5):
        rs.run()
    torch.cuda.synchronize()
    cols = ["prologue", "build", "pro+build", "start->fwdL0 end", "head", "head bwd", "head+bwd", "local total",
            "virt ->L0 reduce", "virt total", "max local", "max virtual",
            "virt L0 begin", "virt L1 begin", "virt L2 begin", "bwd layer 2", "bwd layer 1", "bwd layer 0"]
    out = []
    for _ in range(N):
        buf.zero_()
        rs.run()
        torch.cuda.synchronize()
        st = buf.cpu().numpy()
        l, v = st[g], st[B + g]
        out.append([l[1] - l[0], l[3] - l[1], l[3] - l[0], l[5] - l[0], l[13] - l[12], l[14] - l[13], l[14] - l[12],
                    l[61] - l[0], v[5] - v[0], v[62] - v[0], (st[:B, 61] - st[:B, 0]).max(),
                    (st[B:, 62] - st[B:, 0]).max(), v[4] - v[0], v[8] - v[0], v[12] - v[0],
                    l[22] - l[14], l[19] - l[22], l[16] - l[19]])
    a = np.array(out)
    print(f"graph {g} n={sizes[g]}, {ids}, {N} launches: median (min - max) cycles")
    for j, c in enumerate(cols):
        print(f"   {c:20s} {int(np.median(a[:, j])):7d} ({a[:, j].min():6d} - {a[:, j].max():6d})")


if __name__ == "__main__":
    main()
