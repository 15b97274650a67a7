#!/usr/bin/env python3
"""Write tests/golden/resident_launch_plans.npz from hscn_resident_launch_plan_ex of the library that is loaded:

  python tools/record_resident_plans.py OUT.npz

One int32 row per (launch shape, widths, maxima, want_export): COLUMNS below -- the query's arguments, its return code
and its fields (zeros unless the code is 0).  The committed fixture was recorded from the launch functions of the
commit BEFORE the planners existed (their kernel launches replaced by a recorder of template arguments, grid, threads,
LDS and the argument blocks' choice fields); tests/test_resident_plan_host.py holds the query to it row for row, so
a change to a planner shows as a changed row.  Re-record only for a change that is meant to move a launch choice.

The grid: WIDTHS x _shapes() of tests/test_resident_plan_host.py, and around every size at which a launch takes
another path (EDGES): the 4-wave / 16-wave classes, the caps of the step's compile-time layouts, the buffer, weight
and export switches of the pair at H = 32, the step's 81 KB floor."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]

import numpy as np

from tests.test_resident_plan_host import WIDTHS, _shapes

ARGS = ("launch", "F", "H", "L", "C", "max_n", "max_v", "max_ell", "max_evv", "want_export")


def _edges():
    """(F, H, L, C, max_n, max_v, max_ell, max_evv) around the sizes the regular grid does not straddle."""
    out = []
    for F, H, L, C in WIDTHS:
        for n in (64, 65, 448, 449):                                   # thread classes; StepLCaps::N / StepVCaps::N
            for ell in (1024, 1025):                                   # StepLCaps::ELL
                for v, evv in ((32, 528), (33, 528), (32, 529)):       # StepVCaps::V / ::EVV
                    out.append((F, H, L, C, n, v, ell, evv))
    for L in (2, 3, 4):                                                # StepLCaps::L / ::C at H = 16
        for C in (16, 17):
            for n in (65, 444, 448, 449):
                out.append((9, 16, L, C, n, 8, 1000, 36))
    for n in (337, 338, 384, 385, 439, 440):                           # H = 32: three / two buffers, db, the export
        for L in (2, 3):                                               # (edges: a tree + n // 8 chords, as the trees
            out.append((9, 32, L, 3, n, 8, 2 * (n - 1 + n // 8) + 2, 36))  # of tests/test_gpu_resident_f64.py)
    for n in (65, 100, 150, 200, 230, 240, 250, 260, 300):             # the step's LDS below and above the 81 KB floor
        for H in (16, 32):
            out.append((9, H, 2, 10, n, 8, 2 * n, 36))
    return out


def grid():
    shapes = [(F, H, L, C, n, v, ell, evv) for F, H, L, C in WIDTHS for n, v, ell, evv in _shapes()] + _edges()
    for launch in range(4):
        for s in shapes:
            for want in (0, 1):
                yield (launch,) + s + (want,)


def rows(query):
    """query(launch, F, H, L, C, max_n, max_v, max_ell, max_evv, want_export) -> (rc, fields)"""
    out = []
    for a in grid():
        rc, fields = query(*a)
        out.append(list(a) + [rc] + list(fields))
    return np.asarray(out, dtype=np.int32)


def columns():
    from graph_hscn import _hip
    return ARGS + ("rc",) + _hip.PLAN_FIELDS_EX


def main():
    from graph_hscn import _hip
    r = rows(_hip.resident_launch_plan_ex)
    np.savez_compressed(sys.argv[1], rows=r, columns=np.array(columns()))
    ok = r[r[:, len(ARGS)] == 0]
    print(f"{len(r)} rows, {len(ok)} supported", flush=True)


if __name__ == "__main__":
    main()
