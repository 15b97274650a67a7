"""The one-launch step (csrc/resident_step.h) at the edges of its in-LDS structure builds:

  * the local program's 16-byte row records (csrc/resident_common.h, build_ell16_pair): an edge leaves the packed key
    ``edge number << 16 | neighbour id`` in the slot it draws, the row's thread sorts the six keys through a comparator
    network (csrc/row_sort6.h) and masks the ids out;
  * the virtual program's CSRs of the local->virtual relation (a ballot multisplit over 64-edge chunks) and of the
    virtual->virtual relation (the general build).  These two are as they were when the fixtures were recorded; their
    cases hold them in place for a two-barrier split of both, which must reproduce the bits.

A build decides only HOW the same stable structure (every row's neighbours in ascending edge order, the degree norms)
is produced; no sum and no rounding depends on it.  So every case is held, bit for bit,

  (a) to ``tests/golden/step_bits_builds_<case>.npz``: prediction, score, every gradient, the loss and the final virtual
      features of the one-launch step of the commit BEFORE the packed-key records on the same inputs on an MI355X
      (``tools/record_step_bits.py OUTDIR tests.test_gpu_step_builds`` wrote them);
  (b) to the same step run with ``structure="batch"``: it loads the structure that ``engine.build_structure`` makes
      with the hscn_resident_structure kernels (csrc/structure.hip), which share no code with the builds in LDS.

From outside nothing tells the record build from its fallback, the general CSR build: both give the same bits, which is
the point.  Which one a workgroup takes follows from its graph alone (a row of more than six edges, or more than 65 535
edges or rows); the cases assert that property on the host batch and the launch form through ``step_variant``.

Cases (H = 16, F = 9, C = 10, cross-entropy, float storage and L = 3 unless the case says otherwise; a batch of three
graphs: the one the case is named for, then chains with chords of 33 and 17 nodes, K = 8 clusters):

  deg6_shuffled    n = 70, arcs i -> i +- 1, 2, 3 (mod n): every row holds exactly 6 in- and 6 out-edges; the edge list in
                   a seeded random order, so slots are drawn out of order and the network must permute
  deg7             the same plus one arc: one row of 7 in either table -> that workgroup takes the general build, the
                   other two graphs the records
  dups_loops       a chain with an arc stored twice, a self-loop and two isolated nodes (c = 0: norm 0, a record of
                   the row itself only)
  n1               a graph of one node and no edge (with its batch of 33 and 17 nodes: 4-wave workgroups)
  cap_fixed        n = 448 with 1 024 edges: the caps of the compile-time layout; the key fields reach edge number 1 023
                   and id 447
  runtime_big      n = 513 with more than 1 024 edges, L = 2: the run-time layout (three layers of such a graph are more
                   than a CU's LDS holds)
  w4_deg6          n = 64, 33, 17 with rows of 6 in the first: 4-wave workgroups
  f16_deg6         deg6_shuffled in half storage
  one_cluster_448  K = 1, n = 448: one lv row over seven 64-edge chunks
  k32_interleaved  K = 32, n = 160, cluster ids i % 32: each of the three chunks holds every key
  straddle         K = 3, n = 192: clusters of 63 / 64 / 65 members, interleaved across the chunk borders
  hole             cluster 2 of 8 has no member: an empty lv row between used ones
  vv_k16_complete  K = 16, every ordered pair of distinct clusters: 240 vv edges
  vv_k32_complete  K = 32, 992 vv edges: past StepVCaps::EVV = 528, the run-time layout of the virtual program
  novv             the first graph has no vv edge"""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_step_layouts import step_bits, step_variant  # noqa: F401  (the recorder takes them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, F, C = 16, 9, 10
# name -> (first graph's size, K, L, storage type)
SHAPES = {
    "deg6_shuffled": (70, 8, 3, "f32"),
    "deg7": (70, 8, 3, "f32"),
    "dups_loops": (70, 8, 3, "f32"),
    "n1": (1, 8, 3, "f32"),
    "cap_fixed": (448, 8, 3, "f32"),
    "runtime_big": (513, 8, 2, "f32"),
    "w4_deg6": (64, 8, 3, "f32"),
    "f16_deg6": (70, 8, 3, "f16"),
    "one_cluster_448": (448, 1, 3, "f32"),
    "k32_interleaved": (160, 32, 3, "f32"),
    "straddle": (192, 3, 3, "f32"),
    "hole": (100, 8, 3, "f32"),
    "vv_k16_complete": (100, 16, 3, "f32"),
    "vv_k32_complete": (100, 32, 3, "f32"),
    "novv": (100, 8, 3, "f32"),
}
CASES = list(SHAPES)
REST = (33, 17)                    # the batch's other two graphs

# The launch form of each case, from the planner's rules (csrc/resident_kernels.h, plan_step): 4-wave workgroups up to
# 64 nodes, else 16 waves; the virtual program's layout at compile time within StepVCaps (n <= 448, <= 32 clusters,
# <= 528 vv edges); the local program's beside it within StepLCaps (n <= 448, <= 1024 ll edges, L = 3, C <= 16).
EXPECTED = {name: dict(threads=1024, local_fixed=1, virtual_fixed=1) for name in CASES}
EXPECTED["w4_deg6"] = EXPECTED["n1"] = dict(threads=256, local_fixed=0, virtual_fixed=0)
EXPECTED["runtime_big"] = EXPECTED["vv_k32_complete"] = dict(threads=1024, local_fixed=0, virtual_fixed=0)


def case_id(case):
    return f"builds_{case}"


def _chain(n):
    """A chain with a chord every 5 nodes, both directions stored: rows of at most 6 edges."""
    src = list(range(n - 1)) + list(range(0, n - 5, 5))
    dst = list(range(1, n)) + list(range(4, n - 1, 5))
    e = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    return np.concatenate([e, e[::-1]], 1)


def _circulant6(n):
    """Arcs i -> i + d (mod n) for d = +-1, +-2, +-3: every node has exactly 6 in- and 6 out-edges."""
    i = np.arange(n, dtype=np.int64)
    return np.concatenate([np.stack([i, (i + d) % n]) for d in (1, 2, 3, -1, -2, -3)], 1)


def _ll_edges(case, n):
    if case in ("deg6_shuffled", "f16_deg6", "w4_deg6"):
        return _circulant6(n)
    if case == "deg7":
        return np.concatenate([_circulant6(n), np.array([[0], [10]], dtype=np.int64)], 1)
    if case == "dups_loops":
        e = _chain(n - 2)                                           # nodes n - 2 and n - 1 stay isolated
        return np.concatenate([e, np.array([[3, 3, 5], [4, 4, 5]], dtype=np.int64)], 1)   # (3 -> 4 is in the chain too)
    if case == "n1":
        return np.zeros((2, 0), dtype=np.int64)
    if case in ("cap_fixed", "one_cluster_448"):
        i = np.arange(n - 1, dtype=np.int64)
        a = np.arange(0, 5 * 65, 5, dtype=np.int64)                 # 447 + 65 = 512 pairs, both directions: 1 024 edges
        e = np.concatenate([np.stack([i, i + 1]), np.stack([a, a + 4])], 1)
        return np.concatenate([e, e[::-1]], 1)
    return _chain(n)


def _cluster_ids(case, rng, n, K):
    if case == "k32_interleaved":
        return np.arange(n) % K
    if case == "straddle":
        return rng.permutation(np.repeat(np.arange(3), (63, 64, 65)))
    return rng.permutation(np.arange(n) % K)                        # every cluster used, sizes within one of each other


def _graph(rng, e, n):
    from graph_hscn.data import Data
    e = e[:, rng.permutation(e.shape[1])]                           # edge order is part of the result: a seeded one
    x = torch.from_numpy((rng.integers(0, 5, (n, F)) / 4.0).astype(np.float32))     # exact in half storage
    y = torch.from_numpy((rng.random((1, C)) < 0.4).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=y, num_nodes=n)


def build_case(case, dev="cuda:0"):
    """-> (model, device batch, host batch); deterministic in ``case`` alone."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import LV, VV, hetero_from_clusters
    from graph_hscn.model.hscn import HSCN
    n0, K, L, dt = SHAPES[case]
    rng = np.random.default_rng(9100 + CASES.index(case))
    hs = []
    for i, n in enumerate((n0,) + REST):
        first = i == 0
        g = _graph(rng, _ll_edges(case, n) if first else _chain(n), n)
        h = hetero_from_clusters(g, _cluster_ids(case if first else "", rng, n, K), K)
        U = int(h["virtual"].num_nodes)
        if first and case == "hole":                                # cluster 2's members join cluster 3: row 2 is empty
            lv = h[LV].edge_index.clone()
            lv[1][lv[1] == 2] = 3
            h[LV].edge_index = lv
        if first and case in ("vv_k16_complete", "vv_k32_complete"):
            a, b = np.meshgrid(np.arange(U), np.arange(U), indexing="ij")
            keep = a != b
            vv = np.stack([a[keep], b[keep]]).astype(np.int64)
            h[VV].edge_index = torch.from_numpy(vv[:, rng.permutation(vv.shape[1])])
        if first and case == "novv":
            h[VV].edge_index = torch.zeros(2, 0, dtype=torch.int64)
        hs.append(h)
    host = HeteroBatch.from_data_list(hs)
    d = host.to(dev)
    if dt == "f16":
        d = d.with_feature_dtype(torch.float16)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.from_numpy((0.3 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    model = model.to(dev)
    model.compute_virtual = True
    return model, d, host


def run_one_launch(model, d, structure=None):
    from graph_hscn.step import ResidentTrainStep
    one = ResidentTrainStep(model, d, "cross_entropy", one_launch=True, structure=structure)
    assert one.one_launch
    one.run()
    one.run()                     # buffers are rewritten, not accumulated into
    torch.cuda.synchronize()
    one.check()
    return one


def check_structure(case, host):
    """The property of the host batch the case is named for (first graph)."""
    from graph_hscn import engine
    n0, K, L, dt = SHAPES[case]
    n_local = np.diff(host["local"].ptr.numpy())
    n_virt = np.diff(host["virtual"].ptr.numpy())
    assert tuple(n_local) == (n0,) + REST
    ll = host.edge_index_dict[engine.LL].numpy()
    first = ll[:, (ll[1] < n0)]
    indeg = np.bincount(first[1], minlength=n0)
    outdeg = np.bincount(first[0], minlength=n0)
    rest_in = np.bincount(ll[1], minlength=int(n_local.sum()))[n0:]
    assert int(rest_in.max()) <= 6                                  # the other two graphs always take the records
    if case in ("deg6_shuffled", "f16_deg6", "w4_deg6"):
        assert (indeg == 6).all() and (outdeg == 6).all()
        assert not (np.diff(first[1]) >= 0).all()                   # (rows' edges do not come in slot order)
    elif case == "deg7":
        assert sorted(indeg)[-2:] == [6, 7] and sorted(outdeg)[-2:] == [6, 7]
    else:
        assert int(indeg.max()) <= 6 and int(outdeg.max()) <= 6
    if case == "dups_loops":
        pairs = first[0] * n0 + first[1]
        assert int((pairs == 3 * n0 + 4).sum()) == 3 and int((first[0] == first[1]).sum()) == 1
        assert (indeg[-2:] == 0).all() and (outdeg[-2:] == 0).all()
    if case == "n1":
        assert first.shape[1] == 0
    if case == "cap_fixed":
        assert first.shape[1] == 1024 and int(first.max()) == 447
    if case == "runtime_big":
        assert first.shape[1] > 1024
    lv = host.edge_index_dict[engine.LV].numpy()
    members = np.bincount(lv[1][lv[0] < n0], minlength=int(n_virt[0]))
    if case == "one_cluster_448":
        assert tuple(members) == (448,)
    ids = lv[1][lv[0] < n0]                                         # the first graph's keys in edge order
    if case == "k32_interleaved":
        assert all(len(set(ids[c:c + 64])) == 32 for c in range(0, n0, 64))
    if case == "straddle":
        assert sorted(members) == [63, 64, 65]
        assert all(len(set(ids[c:c + 64])) == 3 for c in range(0, n0, 64))
    if case == "hole":
        assert int(n_virt[0]) == 8 and members[2] == 0 and (np.delete(members, 2) > 0).all()
    vv = host.edge_index_dict[engine.VV].numpy()
    nvv = int((vv[0] < int(n_virt[0])).sum())
    if case == "vv_k16_complete":
        assert int(n_virt[0]) == 16 and nvv == 240
    if case == "vv_k32_complete":
        assert int(n_virt[0]) == 32 and nvv == 992
    if case == "novv":
        assert nvv == 0 and vv.shape[1] > 0


_memo = {}


def _run(case):
    """The case's two steps, run once and shared by its tests: (host batch, launch form, bits in LDS, bits loaded)."""
    if case not in _memo:
        from graph_hscn.engine import build_structure
        model, d, host = build_case(case)
        one = run_one_launch(model, d)
        assert one.virtual is not None and one.idle_cus
        build_structure(d)
        loaded = run_one_launch(model, d, structure="batch")
        assert loaded.structure is d.structure
        _memo[case] = (host, step_variant(one), step_bits(one), step_bits(loaded))
    return _memo[case]


@pytest.mark.parametrize("case", CASES)
def test_step_builds_match_parent_bits(case):
    host, variant, got, _ = _run(case)
    check_structure(case, host)
    assert variant == EXPECTED[case], "the case runs the launch form it is named for"
    assert np.isfinite(got["grads"]).all() and float(np.abs(got["grads"][:-1]).max()) > 0
    with np.load(os.path.join(GOLDEN, f"step_bits_{case_id(case)}.npz")) as gold:
        assert sorted(gold.files) == sorted(got)
        for k in got:
            assert got[k].shape == gold[k].shape and got[k].tobytes() == gold[k].tobytes(), k


@pytest.mark.parametrize("case", CASES)
def test_step_builds_match_loaded_structure(case):
    _, _, got, loaded = _run(case)
    assert sorted(got) == sorted(loaded)
    for k in got:
        assert got[k].tobytes() == loaded[k].tobytes(), k
