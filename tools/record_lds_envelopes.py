#!/usr/bin/env python3
"""Write tests/golden/lds_envelopes.npz from the hscn_*_supported functions of the library that is loaded:

  python tools/record_lds_envelopes.py OUT.npz

One int32 array per function, a row per call: its arguments (ARGS of the test) and its answer.  The committed fixture was
recorded from the commit BEFORE the launch sites shared one helper and the named LDS limits;
tests/test_lds_envelope_host.py holds the functions to it row for row, so a limit that moves shows as a changed row.
Re-record only for a change that is meant to move an envelope.

The grid, per function: the hidden width in {16, 32} and one refused width; two edge counts per node count (2 n and
8 n); for stage A, K in {4, 16, 64}; max_n at every 16th value up to MAX_N and at every value within 8 of a change of
the answer, so both sides of each LDS limit are present to the node."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

import numpy as np

from tests.test_lds_envelope_host import ARGS

MAX_N = 1280
WIDTHS = (16, 32, 24)
EDGES_PER_NODE = (2, 8)


def groups(name):
    """Callables (n, e) -> argument tuple, one per combination of the fixed arguments."""
    for H in WIDTHS:
        if name.startswith("hscn_scn"):
            for K in (4, 16, 64):
                yield lambda n, e, H=H, K=K: (9, H, K, n, e)
        elif name == "hscn_mpnn_supported":
            yield lambda n, e, H=H: (9, H, 3, 10, n, e)
        elif name == "hscn_vl_supported":
            yield lambda n, e, H=H: (9, H, 2, 10, n, 8, e, 36)
        else:   # SignNet's widths are hidden / phi_out; 65 is the refused one
            W = 65 if H == 24 else H
            yield lambda n, e, W=W: (0, 0, 9, 8, W, W, 2, 2, 8, 9, n, e)


def rows(fn, name):
    out = []
    for g in groups(name):
        for per_node in EDGES_PER_NODE:
            ans = [fn(*g(n, per_node * n)) for n in range(MAX_N + 1)]
            change = [n for n in range(1, MAX_N + 1) if ans[n] != ans[n - 1]]
            for n in range(MAX_N + 1):
                if n % 16 == 0 or any(abs(n - c) <= 8 for c in change):
                    out.append(list(g(n, per_node * n)) + [ans[n]])
    return np.asarray(out, dtype=np.int32)


def main():
    from graph_hscn import _hip
    lib = _hip.lib()
    arrays = {name: rows(getattr(lib, name), name) for name in ARGS}
    np.savez_compressed(sys.argv[1], **arrays)
    for name, r in arrays.items():
        print(f"{name}: {len(r)} rows, {int(r[:, -1].sum())} supported", flush=True)


if __name__ == "__main__":
    main()
