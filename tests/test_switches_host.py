"""Every switch the sources read is listed here, and every run-time switch of the C library is named by a test.

A kernel keeps one code path unless a test pins the other one: the ``getenv`` knobs of the host launchers, the
``#if`` / ``#ifdef`` / ``#ifndef`` macros of the kernel sources and the ``os.environ`` reads of the Python package are
scanned and compared with the three explicit sets below ("Switches", says what each one selects).  A
new knob therefore fails this file until it is added here AND -- on the C side -- some other test file names it.
``HSCN_STAMPS`` is the one compile-time macro: the stamped diagnostic build of ``make diag`` (tools/diag_*.py), never
shipped and never timed, so no GPU test builds it."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graph-hscn_amd", "csrc")
PKG = os.path.join(ROOT, "graph-hscn_amd", "graph_hscn")

C_GETENV = {
    "HSCN_LINEAR_BWD_W",
    "HSCN_SPMM_PIPE", "HSCN_SPMM_NV", "HSCN_SPMM_PASSES",
    "HSCN_DENSE_AS", "HSCN_DENSE_ROWS",
    "HSCN_PERSISTENT_EPOCH",
    "HSCN_ALLREDUCE_FORM",
}
C_MACROS = {"HSCN_STAMPS"}
PY_ENVIRON = {
    "HSCN_DENSE_ADJ",                                   # a test runs it
    "HSCN_LIB", "HSCN_ALLREDUCE", "HSCN_COMM_MEMORY",   # configuration
    "HSCN_ONE_LAUNCH", "HSCN_OVERLAP_VIRTUAL",          # issue forms the suite tests through arguments / attributes
}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _scan(paths, pattern):
    found = {}
    for p in paths:
        for m in re.finditer(pattern, _read(p), re.M):
            for name in re.findall(r"HSCN_\w+", m.group(0)):
                found.setdefault(name, set()).add(os.path.relpath(p, ROOT))
    return found


def test_the_switches_of_the_sources_are_exactly_the_listed_ones():
    csrc = sorted(glob.glob(os.path.join(CSRC, "*")))
    assert csrc, CSRC
    getenv = _scan(csrc, r'getenv\s*\(\s*"HSCN_\w+"')
    macros = _scan(csrc, r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b[^\n]*HSCN_\w+[^\n]*")
    py = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert py, PKG
    environ = _scan(py, r"""os\s*\.\s*(?:environ\s*(?:\.\s*(?:get|pop|setdefault)\s*\(|\[)|getenv\s*\()\s*["']HSCN_\w+""")
    assert set(getenv) == C_GETENV, {n: sorted(getenv[n]) for n in set(getenv) ^ C_GETENV if n in getenv}
    assert set(macros) == C_MACROS, {n: sorted(macros[n]) for n in set(macros) ^ C_MACROS if n in macros}
    assert set(environ) == PY_ENVIRON, {n: sorted(environ[n]) for n in set(environ) ^ PY_ENVIRON if n in environ}


def test_every_switch_of_the_c_library_is_named_by_a_test():
    here = os.path.abspath(__file__)
    tests = [p for p in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)]
    everywhere = "\n".join(_read(p) for p in tests)
    elsewhere = "\n".join(_read(p) for p in tests if os.path.abspath(p) != here)
    for name in sorted(C_GETENV | C_MACROS):
        assert re.search(rf"\b{name}\b", everywhere), name
    for name in sorted(C_GETENV):          # a run-time knob is exercised by a test other than this list
        assert re.search(rf"\b{name}\b", elsewhere), f"{name}: no test sets it"
