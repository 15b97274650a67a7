"""Exphormer's typed sparse attention (csrc/exphormer.hip) gives, bit for bit, what the commit before its head-unit
helpers moved into csrc/row_walk.h gave: the forward's ``out`` and ``z`` and every gradient of the four backward passes.

tests/golden/exphormer_bits.npz was recorded from that commit's library
(``HSCN_LIB=<its libhscn.so> python tools/record_step_bits.py OUTDIR tests.test_gpu_exphormer_bits``) on the inputs built
here, in the style of tests/test_gpu_row_walk_bits.py: every tensor is held as the SHA-256 of the int32 view of its
float32 storage under the name ``<case>/<tensor>``.  Equal bytes or a failure.

The cases cross (heads, C) -- (1, 4): G = 1;  (3, 3): VEC = 1;  (2, 40): G = 16 with idle lanes;  (1, 512): G = 64 and
two column passes;  (4, 16) with q at a 4-byte offset: VEC = 1 at a width that would take 16-byte lanes -- with and
without per-edge feature rows (``e_edge``) and with nv = 0 and nv = 1 (two and four edge types).

Every case runs one union graph (``_graph``) whose target rows 0 .. 7 have 0, 1, 3, 4, 5, 9, 256 and 257 in-edges and
whose source rows have the same out-degrees, so both the target-keyed and the source-keyed walk meet: the look-ahead of
XA_AHEAD = 4 slots and its remainder loop (0 .. 9), ROW_WALK_LONG_ROW and one over it (256, 257), and at G = 64 -- four
lane groups per workgroup -- the 257-slot row as 64 * UPB + 1 slots: five chunks, a second merge round.  With per-edge
rows the typed edges are 64 of type 0 and 65 of type 1 (EXPH_TYPE_LONG_ROW and one over it; with nv = 1 three more of
type 2 and none of type 3, whose gradient is exact zeros); without them every edge is typed and every type is split
into many chunks."""
import hashlib
import os

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import ExphormerStructure
from tests.helpers import DEV

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exphormer_bits.npz")
DEGREES = (0, 1, 3, 4, 5, 9, 256, 257)
FEEDERS = 11
WIDTHS = ((1, 4, False), (3, 3, False), (2, 40, False), (1, 512, False), (4, 16, True))     # (heads, C, q misaligned)
CASES = [(h, c, off, with_e, nv) for (h, c, off) in WIDTHS for with_e in (True, False) for nv in (0, 1)]
TENSORS = ("out", "z", "dq", "dk", "dv", "de_edge", "de_type")


def case_id(case):
    heads, C, off, with_e, nv = case
    return f"h{heads}_c{C}{'_qoff' if off else ''}_{'edge' if with_e else 'typed'}_nv{nv}"


def _graph(with_e, nv):
    """(edge_index [2, E], erow [E], rows, El): target row i < 8 receives DEGREES[i] edges from the FEEDERS rows after
    the targets in turn; the same list, flipped and moved up by 8 + FEEDERS rows, gives source rows of those
    out-degrees; nv further rows stand last.  Edges in a seeded random order (eid[slot] != slot)."""
    n = len(DEGREES) + FEEDERS
    dst = torch.cat([torch.full((d,), i) for i, d in enumerate(DEGREES)])
    src = len(DEGREES) + torch.arange(dst.numel()) % FEEDERS
    a = torch.stack([src, dst])
    ei = torch.cat([a, a.flip(0) + n], 1)
    g = torch.Generator().manual_seed(2 * int(with_e) + nv)
    E, T = ei.size(1), 2 + 2 * nv
    ei = ei[:, torch.randperm(E, generator=g)].contiguous()
    if with_e:
        counts = [64, 65] + ([3, 0] if nv else [])
        typed = sum(counts)
        El = E - typed
        erow = torch.cat([torch.randperm(El, generator=g)] + [torch.full((c,), El + t) for t, c in enumerate(counts)])
        erow = erow[torch.randperm(E, generator=g)]
    else:
        El = 0
        erow = torch.randint(0, T, (E,), generator=g)
    return ei, erow, 2 * n + nv, El


def run_case(case):
    """name -> device tensor: the outputs and gradients of the case, on seeded inputs."""
    heads, C, off, with_e, nv = case
    HC = heads * C
    ei, erow, rows, El = _graph(with_e, nv)
    T = 2 + 2 * nv
    g = torch.Generator().manual_seed(100 + CASES.index(case))
    x = [torch.randn(rows, HC, generator=g) for _ in range(3)]
    x += [0.5 * torch.randn(El, HC, generator=g) if El else None, 0.5 * torch.randn(T, HC, generator=g)]
    go = torch.randn(rows, HC, generator=g).to(DEV)
    q, k, v, e_edge, e_type = [None if t is None else t.to(DEV).requires_grad_(True) for t in x]
    if off:                                     # q at a 4-byte offset: every pass takes the VEC = 1 path
        flat = torch.zeros(q.numel() + 1, device=DEV)
        flat[1:] = x[0].to(DEV).flatten()
        q = flat[1:].view(rows, HC).requires_grad_(True)
        assert q.data_ptr() % 16 == 4 and q.is_contiguous()
    struct = ExphormerStructure.from_parts(ei.to(DEV), erow.to(DEV), rows - nv, 1, nv, El)
    out = Fh.ExphormerAttentionFn.apply(q, k, v, e_edge, e_type, struct, heads)
    z = out.grad_fn.saved_tensors[6]
    out.backward(go)
    struct.rel.check()
    torch.cuda.synchronize()
    got = {"out": out, "z": z, "dq": q.grad, "dk": k.grad, "dv": v.grad, "de_type": e_type.grad}
    if El:
        got["de_edge"] = e_edge.grad
    assert tuple(z.shape) == (rows, heads)
    assert all(t is not None and t.dtype == torch.float32 for t in got.values()), case_id(case)
    return got, struct


def digest(t):
    """SHA-256 of the tensor's bits (the int32 view of its float32 storage, row-major)."""
    return hashlib.sha256(t.detach().contiguous().view(torch.int32).cpu().numpy().tobytes()).digest()


def record_bits(outdir):
    """tools/record_step_bits.py: write the fixture from the library that is loaded."""
    names, digests = [], []
    for case in CASES:
        for k, t in sorted(run_case(case)[0].items()):
            names.append(f"{case_id(case)}/{k}")
            digests.append(np.frombuffer(digest(t), dtype=np.uint8))
        print(case_id(case), flush=True)
    np.savez_compressed(os.path.join(outdir, "exphormer_bits.npz"), names=np.array(names), sha256=np.stack(digests))
    print(len(CASES), "cases,", len(names), "digests")


_golden = {}


def _recorded():
    if not _golden:
        z = np.load(GOLDEN)
        _golden.update({str(n): bytes(d) for n, d in zip(z["names"], z["sha256"])})
    return _golden


def test_the_cases_are_distinct_and_the_fixture_names_every_tensor_of_them():
    assert len({case_id(c) for c in CASES}) == len(CASES)
    want = {f"{case_id(c)}/{k}" for c in CASES for k in TENSORS if k != "de_edge" or c[3]}
    assert set(_recorded()) == want


def test_the_graph_has_the_rows_the_cases_are_about():
    L = _hip.lib()
    long_row, chunk = L.hscn_exph_attn_long_row(), L.hscn_exph_attn_chunk()
    assert (long_row, long_row + 1) == DEGREES[-2:] and chunk * (256 // 64) + 1 == DEGREES[-1]    # UPB = 4 at G = 64
    for with_e in (True, False):
        for nv in (0, 1):
            ei, erow, rows, El = _graph(with_e, nv)
            n = len(DEGREES) + FEEDERS
            assert torch.bincount(ei[1], minlength=rows)[:len(DEGREES)].tolist() == list(DEGREES)
            assert torch.bincount(ei[0], minlength=rows)[n:n + len(DEGREES)].tolist() == list(DEGREES)
            if with_e:
                types = torch.bincount(erow[erow >= El] - El, minlength=2 + 2 * nv).tolist()
                assert types[:2] == [L.hscn_exph_type_long_row(), L.hscn_exph_type_long_row() + 1]
                assert bool((erow[erow < El] != torch.arange(El)).any())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_before_the_shared_head_unit_layer(case):
    got, struct = run_case(case)
    want = {n.split("/")[1]: d for n, d in _recorded().items() if n.split("/")[0] == case_id(case)}
    assert set(got) == set(want), (sorted(got), sorted(want))
    differ = [k for k in sorted(got) if digest(got[k]) != want[k]]
    assert not differ, f"{case_id(case)}: {differ} differ from the recorded bits"
    longest = [int(c.rowptr.diff().max()) for c in (struct.rel.csr, struct.rel.csr_t)]
    assert longest == [DEGREES[-1], DEGREES[-1]]
