"""The row-walk operators (csrc/gine.hip, gatedgcn.hip, edge_attention.hip) and the two GAT families (csrc/gat.hip,
gat_loops.hip) give, bit for bit, what the commit before they moved onto the shared helpers of csrc/row_walk.h gave.

tests/golden/row_walk_bits.npz was recorded from that commit's library
(``HSCN_LIB=<its libhscn.so> python tools/record_step_bits.py OUTDIR tests.test_gpu_row_walk_bits``) on the inputs built
here.  The tensors of the narrow gine cases of 1. (seven nodes, widths 16 and 17: 128 tensors, 54 kB) are kept whole
and compared with ``torch.equal`` on the int32 view; every other output and gradient is held as the SHA-256 of its
bytes under the name ``<case>/<tensor>``: the 100 cases have 580 tensors of several megabytes together (the two
[E, 260] tensors of one GatedGCN case alone are 550 kB) -- random mantissas, which do not compress -- and the fixture
stays below the largest file of tests/golden/ (100 kB).  A digest is no weaker a comparison: equal bytes or a failure.

The cases (CASES below) cross every branch of the two-phase long-row skeleton:
  1. degrees around the split: one hub row of 256, 257, 320 or 321 slots (at and one over ROW_WALK_LONG_ROW, then whole
     chunks and a last chunk of one slot) among six short rows of degree 0, 1 and 3, the hub as target (the
     target-keyed walks split it) and as source (the source-keyed walks do); widths 16 (16-byte lanes) and 17 (scalar
     lanes, idle lanes at the block's end); gine with De = 3 and 9 (weights in registers / read per edge), GatedGCN,
     edge attention with (heads, C) = (2, 8) and edge features and (1, 10) without;
  2. two rounds of chunks (more chunks than lane groups in a block);
  3. two column passes of gine and GatedGCN (widths 260 and 67), with short rows only and with a 257-slot hub;
  4. GATConvFn and GATLoopFn (both kernel families) on the graph of 1. with 257 slots, once with listed self loops.
GatedGCN and edge attention also run the backward in which the target walk takes every row as empty (``walk == 0``).

The one case whose output is too large for a fixture -- the tile loops' second trip, with the long row on it -- is held
to the float64 referee of tests/test_gpu_gine.py instead (``test_grid_stride_with_a_long_row_on_the_second_trip``)."""
import hashlib
import os

import numpy as np
import pytest
import torch

from graph_hscn.nn import functional as Fh
from graph_hscn.structure import Relation, with_self_loops
from tests.helpers import DEV
from tests.test_gpu_gine import _check_forward, _inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_walk_bits.npz")
N_NODES, HUB = 7, 3
SPLIT_DEGREES = (256, 257, 320, 321)


# --------------------------------------------------------------------------- #
# cases: (operator, shape, hub degree or None, "target" | "source")
# --------------------------------------------------------------------------- #
def _cases():
    out = []
    for hub in ("target", "source"):
        for d in SPLIT_DEGREES:                                              # 1.
            for F in (16, 17):
                out += [("gine", (F, 3), d, hub), ("gine", (F, 9), d, hub), ("gated", (F,), d, hub)]
            out += [("ea", (2, 8, True), d, hub), ("ea", (1, 10, False), d, hub)]
        for op in ("gine", "gated"):                                         # 2. and 3.
            sh = (lambda F: (F, 3)) if op == "gine" else (lambda F: (F,))
            out += [(op, sh(128), 768, hub), (op, sh(17), 1024, hub)]
            out += [(op, sh(F), d, hub) for F in (260, 67) for d in (None, 257)]
        out += [("ea", (1, 10, False), 1088, hub), ("ea", (1, 128, False), 768, hub)]
    for F in (16, 17):                                                       # 4.
        out += [("gat", (F,), 257, "target"), ("gat_narrow", (F,), 257, "target"), ("gat_wide", (F,), 257, "target")]
    out += [("gat_narrow", (16, "loops"), 257, "target"), ("gat_wide", (17, "loops"), 257, "target")]
    return out


CASES = _cases()


def case_id(case):
    op, shape, d, hub = case
    return f"{op}_{'x'.join(str(int(s) if not isinstance(s, str) else s) for s in shape)}_d{d}_{hub}"


def _graph(d, hub, loops=False):
    """Seven nodes in random edge order: node 3 receives ``d`` edges from the others in turn (none for d = None); nodes
    1 and 5 have in-degree 1, nodes 2 and 6 in-degree 3 (one edge repeated), nodes 0 and 4 none.  hub = "source": the
    same list with both rows exchanged.  loops: nodes 3 and 5 list a self loop as well."""
    others = torch.tensor([n for n in range(N_NODES) if n != HUB])
    src = others[torch.arange(d or 0) % others.numel()]
    short = torch.tensor([[0, 4, 4, 1, 2, 2, 0, 5], [1, 2, 2, 2, 5, 6, 6, 6]])
    ei = torch.cat([torch.stack([src, torch.full_like(src, HUB)]), short], 1)
    if loops:
        ei = torch.cat([ei, torch.tensor([[3, 5], [3, 5]])], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(ei.size(1)))]
    return (ei if hub == "target" else ei.flip(0)).contiguous()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def _run_gine(shape, rel, E, g):
    F, De = shape
    x, W, b = _leaves(_randn(g, N_NODES, F), _randn(g, F, De) / De ** 0.5, 0.1 * _randn(g, F))
    ea, gz = _randn(g, E, De), _randn(g, N_NODES, F)
    z = Fh.GINEAggregateFn.apply(x, ea, W, b, rel, 0.25)
    z.backward(gz)
    return {"z": z, "gx": x.grad, "gW": W.grad, "gb": b.grad}


def _run_gated(shape, rel, E, g):
    (H,) = shape
    ins = [_randn(g, N_NODES, H) for _ in range(4)] + [_randn(g, E, H)]
    gh, ge = _randn(g, N_NODES, H), _randn(g, E, H)
    leaves = _leaves(*ins)
    h, e_out = Fh.GatedGCNAggregateFn.apply(*leaves, rel)
    torch.autograd.backward([h, e_out], [gh, ge])
    out = {"h": h, "e_out": e_out}
    out.update({"g" + n: t.grad for n, t in zip(("Ax", "Bx", "Dx", "Ex", "Ce"), leaves)})
    only_b = [t.detach().clone().requires_grad_(i == 1) for i, t in enumerate(ins)]     # walk == 0
    Fh.GatedGCNAggregateFn.apply(*only_b, rel)[0].backward(gh)
    out["gBx_alone"] = only_b[1].grad
    return out


def _run_ea(shape, rel, E, g):
    heads, C, with_e = shape
    HC = heads * C
    ins = [_randn(g, N_NODES, HC) for _ in range(3)] + ([_randn(g, E, HC)] if with_e else [])
    go = _randn(g, N_NODES, HC)
    leaves = _leaves(*ins)
    o = Fh.EdgeAttentionFn.apply(leaves[0], leaves[1], leaves[2], leaves[3] if with_e else None, rel, heads)
    o.backward(go)
    out = {"out": o}
    out.update({"d" + n: t.grad for n, t in zip("qkve", leaves)})
    kv = [t.detach().clone().requires_grad_(i in (1, 2)) for i, t in enumerate(ins)]     # walk == 0
    Fh.EdgeAttentionFn.apply(kv[0], kv[1], kv[2], kv[3] if with_e else None, rel, heads).backward(go)
    out.update({"dk_alone": kv[1].grad, "dv_alone": kv[2].grad})
    return out


def _run_gat(op, shape, ei, g):
    H, F_in = shape[0], 9
    n = N_NODES
    rel = Relation(ei, n, n, both=True)
    x, W, a_s, a_d, b = _leaves(_randn(g, n, F_in), _randn(g, H, F_in) / 3.0, _randn(g, 1, 1, H), _randn(g, 1, 1, H),
                                _randn(g, H))
    gy = _randn(g, n, H)
    if op == "gat":                        # bipartite form, two transforms
        xd, Wd = _leaves(_randn(g, n, F_in), _randn(g, H, F_in) / 3.0)
        y = Fh.GATConvFn.apply(x, xd, W, Wd, a_s, a_d, b, rel, 0.2, Fh.ACT["elu"])
        names, leaves = ("x_src", "x_dst", "W_src", "W_dst", "att_src", "att_dst", "bias"), (x, xd, W, Wd, a_s, a_d, b)
    else:                                  # self-loop form: the narrow-row kernels, or gat.hip over explicit loops
        loops = Relation(with_self_loops(ei, n), n, n, both=True) if op == "gat_wide" else None
        y = Fh.GATLoopFn.apply(x, W, a_s, a_d, b, rel, loops, 0.2, Fh.ACT["elu"])
        names, leaves = ("x", "W", "att_src", "att_dst", "bias"), (x, W, a_s, a_d, b)
    y.backward(gy)
    out = {"y": y}
    out.update({"g_" + k: t.grad for k, t in zip(names, leaves)})
    return out


def run_case(case):
    """name -> device tensor: every output and every gradient of the case, on seeded inputs."""
    op, shape, d, hub = case
    g = torch.Generator().manual_seed(CASES.index(case))
    ei = _graph(d, hub, loops="loops" in shape).to(DEV)
    if op in ("gat", "gat_narrow", "gat_wide"):
        out = _run_gat(op, shape, ei, g)
    else:
        rel = Relation(ei, N_NODES, N_NODES, both=True)
        out = {"gine": _run_gine, "gated": _run_gated, "ea": _run_ea}[op](shape, rel, ei.size(1), g)
        assert int(rel.csr.flag.item()) == 0
    torch.cuda.synchronize()
    assert all(t is not None and t.dtype == torch.float32 for t in out.values()), case_id(case)
    return out


def digest(t):
    """SHA-256 of the tensor's bits (the int32 view of its float32 storage, row-major)."""
    return hashlib.sha256(t.detach().contiguous().view(torch.int32).cpu().numpy().tobytes()).digest()


def kept_whole(case):
    """The narrow gine cases of part 1: small enough for the fixture to hold their tensors as they are."""
    return case[0] == "gine" and case[2] in SPLIT_DEGREES and case[1][0] in (16, 17)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def record_bits(outdir):
    """tools/record_step_bits.py: write the fixture from the library that is loaded."""
    names, digests, whole = [], [], {}
    for case in CASES:
        for k, t in sorted(run_case(case).items()):
            if kept_whole(case):
                whole[f"whole/{case_id(case)}/{k}"] = bits(t).numpy()
            else:
                names.append(f"{case_id(case)}/{k}")
                digests.append(np.frombuffer(digest(t), dtype=np.uint8))
        print(case_id(case), flush=True)
    np.savez_compressed(os.path.join(outdir, "row_walk_bits.npz"), names=np.array(names), sha256=np.stack(digests),
                        **whole)
    print(len(CASES), "cases,", len(names), "digests,", len(whole), "whole tensors")


_golden = {}


def _recorded():
    if not _golden:
        z = np.load(GOLDEN)
        _golden.update({str(n): bytes(d) for n, d in zip(z["names"], z["sha256"])})
        _golden.update({k[len("whole/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("whole/")})
    return _golden


def test_the_cases_are_distinct_and_the_fixture_names_every_tensor_of_them():
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert {n.split("/")[0] for n in _recorded()} == {case_id(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_same_bits_as_before_the_shared_helpers(case):
    got = run_case(case)
    want = {n.split("/")[1]: d for n, d in _recorded().items() if n.split("/")[0] == case_id(case)}
    assert set(got) == set(want), (sorted(got), sorted(want))
    assert all(torch.is_tensor(w) == kept_whole(case) for w in want.values())
    differ = [k for k in sorted(got)
              if (not torch.equal(bits(got[k]), want[k]) if kept_whole(case) else digest(got[k]) != want[k])]
    assert not differ, f"{case_id(case)}: {differ} differ from the recorded bits"
    if case[2] is not None and case[0] in ("gine", "gated", "ea"):           # the case does split a row
        rel = Relation(_graph(case[2], case[3]).to(DEV), N_NODES, N_NODES, both=True)
        longest = max(int(c.rowptr.diff().max()) for c in (rel.csr, rel.csr_t))
        assert longest == case[2]


def test_grid_stride_with_a_long_row_on_the_second_trip():
    """gine forward at F = 256: 4 rows per block and at most 8192 blocks, so with 8192 * 4 + 3 nodes block 0 takes a
    second tile, and the only long row (300 slots into the last node) lies on it: the one place where the tile loops of
    both phases run a second trip and where ``any_long`` is raised on it.  Node 0, on block 0's first trip, has two
    in-edges.  Referee and tolerance of tests/test_gpu_gine.py::test_long_rows_forward."""
    F, De, N, d = 256, 3, 8192 * 4 + 3, 300
    assert d > Fh.GINE_LONG_ROW
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, N, (d + 2,), generator=g)
    dst = torch.cat([torch.full((d,), N - 1), torch.zeros(2, dtype=torch.int64)])
    ei = torch.stack([src, dst])[:, torch.randperm(d + 2, generator=g)].contiguous()
    x, ea, W, b = _inputs(N, d + 2, F, De, seed=F + d)
    _check_forward(x, ei, ea, W, b, 0.0, f"GINE forward, long row on the second trip, N={N} F={F}", wrong_rows=True)
