#!/usr/bin/env python3
"""Record the bit-for-bit fixtures of tests/test_gpu_step_layouts.py -- or of the test module named as the second
argument, e.g. tests.test_gpu_step_big_clusters -- from the library that is loaded:

  [HSCN_LIB=<libhscn.so of the commit to record>] python tools/record_step_bits.py OUTDIR [MODULE]

The module provides CASES, case_id, build_case, run_one_launch and step_bits -- or record_bits(OUTDIR), which writes the
module's own fixture (tests.test_gpu_row_walk_bits: row_walk_bits.npz).  Writes OUTDIR/step_bits_<case>.npz
(prediction, score, flat gradients + loss, final virtual features of the one-launch
step on the test's own inputs).  Run it on the build whose results a change must reproduce, then copy the files to
tests/golden/."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "graph-hscn_amd")]
import importlib

import numpy as np

T = importlib.import_module(sys.argv[2] if len(sys.argv) > 2 else "tests.test_gpu_step_layouts")


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    if hasattr(T, "record_bits"):          # a module whose fixture is not one file per case writes it itself
        T.record_bits(out)
        return
    for case in T.CASES:
        model, d, _ = T.build_case(case)
        one = T.run_one_launch(model, d)
        bits = T.step_bits(one)
        np.savez_compressed(os.path.join(out, f"step_bits_{T.case_id(case)}.npz"), **bits)
        print(T.case_id(case), {k: v.shape for k, v in bits.items()}, flush=True)


if __name__ == "__main__":
    main()
