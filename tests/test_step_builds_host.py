"""csrc/row_sort6.h on the host (no GPU): the comparator network behind the one-launch step's 16-byte row records
(csrc/resident_common.h, build_ell16_pair) is plain C++, so tests/step_builds_host.cpp includes it, is compiled with the
host compiler under AddressSanitizer and UBSan where the compiler has them, and checks

  * that all 64 zero-one inputs sort (the zero-one principle: the network sorts every input);
  * on 10^4 random rows of 0 .. 6 packed keys that mask-after-sort gives the ids of the earlier rank-and-route form;
  * that the degree norm's table holds the bits of ``1.0f / sqrtf((float)c)`` for c = 0 .. 6."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "step_builds_host.cpp")
INC = os.path.join(ROOT, "graph-hscn_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_row_sort6_on_the_host(tmp_path):
    cxx = _compiler()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "step_builds_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", INC, SRC, "-o", exe]
    # (the runtimes linked in: a stand-alone program that needs nothing from the environment it is started in)
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static,
                         capture_output=True, text=True)
    if san.returncode != 0:                       # a compiler without the sanitizer runtimes: the plain program
        subprocess.run(base, check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "row_sort6 ok"
