"""The one-launch step (csrc/resident_step.h, csrc/resident_kernels.h), bit for bit, at the edges of how its head and
its virtual program are scheduled:

  * the head's four outer-product partials: the compile-time layout (16 waves, L = 3, C <= 16) writes them from waves
    8 .. 11 behind their row tile of the first backward layer, every other form with all threads in front of the
    backward.  Hence the tile counts around the wave count (those waves own no tile, one tile, and sit beside waves with
    two), the head widths on either side of the compile-time layout (C = 16, 17), the layer counts beside L = 3 and the
    4-wave workgroups;
  * the rows the virtual program's loading waves hold (n = 1 .. 513: one wave's share, the eight registers' share, the
    tail loop beyond it), its layer counts and its cluster shapes (one cluster, 16 and 32 small ones, one of more than
    64 members, no virtual->virtual edge), and half storage: what a rescheduling of that program's phases has to
    reproduce (DESIGN.md section 9 has the forms that were measured on these cases).

All of it is scheduling: no sum and no rounding changes.  So every case is held

  * bit for bit to ``tests/golden/step_bits_phase1_<case>.npz``: prediction, score, every gradient, the loss and the
    final virtual features of the one-launch step of the commit BEFORE these changes on the same inputs on an MI355X
    (``tools/record_step_bits.py OUTDIR tests.test_gpu_step_phase1`` wrote them);
  * to the launch pair and to the CPU oracle with the bounds of tests/test_gpu_step_fronts.py (final virtual features
    bit for bit against the pair; prediction, score and loss by ``pool_order_close``; gradients by
    ``grads_close(rel=1e-5)``; the prediction within ATOL of the oracle's, the virtual features by ``scale_close``; half
    storage: the oracle emulates the rounding points and the bound is 2^-10 of the tensor's magnitude).

Cases (H = 16, F = 9; a batch of 3 graphs each; K = 8 clusters of equal size, C = 10, L = 3, cross-entropy, float
storage unless the case says otherwise):

  n1                  n = 1, 1, 1            one row, no local edge at all (4-wave workgroups)
  n63 n64 n65         n = 63|64|65, 17, 33   K = 1: 4-wave against 16-wave workgroups, one against two softmax chunks
  n448                n = 448, 100, 17       the caps of both compile-time layouts
  n513_L2             n = 513, 17, 33; L = 2 run-time layouts; more than 8 x 256 float4 words of a_1 (the loading waves'
                                             tail loop)
  L1 L2 L4            n = 257, 100, 17       L = 1: no hand-off; L = 2; L = 4: four weight sets, run-time local layout
                                             (L = 3 on the same graphs: tiles_257)
  nv16                n = 100, 70, 33        K = 16: 16 clusters of <= 7 members (DPP-row path of the cluster reduce)
  nv32                n = 100, 70, 33        K = 32: the most clusters the compile-time virtual layout takes
  bigcl               n = 75, 33, 17         the first graph: one cluster of 70 members, one of 5, six ids unused (two
                                             virtual nodes where the other graphs have eight: empty slots)
  novv                n = 100, 33, 17        the first graph has no virtual->virtual edge at all
  f16                 n = 257, 100, 17       half storage
  C1 C16 C17          n = 70, 33, 17         fast head at its narrowest and widest, general head just above
  l1                  n = 70, 33, 17         the other loss kind
  tiles_128 .. _257   n = 128|129|240|241|257, 100, 17
                                             8, 9, 15, 16 and 17 row tiles on 16 waves: waves 8 .. 11, which write the
                                             head partials, own no tile (8 tiles), wave 8 owns one (9), all own one
                                             (15, 16), and wave 0 owns two beside them (17)
  C16_4w              n = 40, 17, 64; C = 16 the widest fast head on a 4-wave workgroup (partials in front of the backward)

``test_replay`` runs one case three times in a row and once more under ``torch.cuda.graph`` replay (the epoch word
advances from launch to launch): every run equals the first.

Each case asserts the launch form it is named for (hscn_resident_launch_plan_ex through ``step_variant``)."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_step_layouts import step_bits, step_variant  # noqa: F401  (the recorder takes them from here)
from tests.test_gpu_step_fronts import run_one_launch  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, F = 16, 9
# name -> (graph sizes, K, C, L, loss, storage type)
SHAPES = {
    "n1": ((1, 1, 1), 8, 10, 3, "cross_entropy", "f32"),
    "n63": ((63, 17, 33), 1, 10, 3, "cross_entropy", "f32"),
    "n64": ((64, 17, 33), 1, 10, 3, "cross_entropy", "f32"),
    "n65": ((65, 17, 33), 1, 10, 3, "cross_entropy", "f32"),
    "n448": ((448, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "n513_L2": ((513, 17, 33), 8, 10, 2, "cross_entropy", "f32"),
    "L1": ((257, 100, 17), 8, 10, 1, "cross_entropy", "f32"),
    "L2": ((257, 100, 17), 8, 10, 2, "cross_entropy", "f32"),
    "L4": ((257, 100, 17), 8, 10, 4, "cross_entropy", "f32"),
    "nv16": ((100, 70, 33), 16, 10, 3, "cross_entropy", "f32"),
    "nv32": ((100, 70, 33), 32, 10, 3, "cross_entropy", "f32"),
    "bigcl": ((75, 33, 17), 8, 10, 3, "cross_entropy", "f32"),
    "novv": ((100, 33, 17), 8, 10, 3, "cross_entropy", "f32"),
    "f16": ((257, 100, 17), 8, 10, 3, "cross_entropy", "f16"),
    "C1": ((70, 33, 17), 8, 1, 3, "cross_entropy", "f32"),
    "C16": ((70, 33, 17), 8, 16, 3, "cross_entropy", "f32"),
    "C17": ((70, 33, 17), 8, 17, 3, "cross_entropy", "f32"),
    "l1": ((70, 33, 17), 8, 10, 3, "l1", "f32"),
    "tiles_128": ((128, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_129": ((129, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_240": ((240, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_241": ((241, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_257": ((257, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "C16_4w": ((40, 17, 64), 8, 16, 3, "cross_entropy", "f32"),
}
CASES = list(SHAPES)
TILES = {"tiles_128": 8, "tiles_129": 9, "tiles_240": 15, "tiles_241": 16, "tiles_257": 17}

# The launch form of each case, from the planner's rules (csrc/resident_kernels.h, plan_step): 4-wave workgroups up to
# 64 nodes, else 16 waves; the virtual program's layout at compile time within StepVCaps (n <= 448, <= 32 clusters); the
# local program's beside it within StepLCaps (n <= 448, <= 1024 ll edges, L = 3, C <= 16).
EXPECTED = {name: dict(threads=1024, local_fixed=1, virtual_fixed=1) for name in CASES}
for _c in ("n1", "n63", "n64", "C16_4w"):
    EXPECTED[_c] = dict(threads=256, local_fixed=0, virtual_fixed=0)
EXPECTED["n513_L2"] = dict(threads=1024, local_fixed=0, virtual_fixed=0)
for _c in ("C17", "L1", "L2", "L4"):
    EXPECTED[_c] = dict(threads=1024, local_fixed=0, virtual_fixed=1)


def case_id(case):
    return f"phase1_{case}"


def _graph(rng, n, C, loss):
    """A chain with a chord every 16 nodes, both directions stored: molecule-like rows (at most 4 edges) and at most
    2.2 n edges, so that n = 448 stays within StepLCaps' 1024 edges.  n = 1: no edge."""
    from graph_hscn.data import Data
    src = list(range(n - 1))
    dst = list(range(1, n))
    for a in range(0, n - 7, 16):
        src.append(a)
        dst.append(a + 6)
    e = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    e = np.concatenate([e, e[::-1]], 1)
    e = e[:, rng.permutation(e.shape[1])]                       # edge order is part of the result: fix an arbitrary one
    x = torch.from_numpy((rng.integers(0, 5, (n, F)) / 4.0).astype(np.float32))     # exact in half storage
    if loss == "l1":
        y = torch.from_numpy(rng.standard_normal((1, C)).astype(np.float32))
    else:
        y = torch.from_numpy((rng.random((1, C)) < 0.4).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=y, num_nodes=n)


def build_case(case, dev="cuda:0"):
    """-> (model, device batch, host batch); deterministic in ``case`` alone."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import VV, hetero_from_clusters
    from graph_hscn.model.hscn import HSCN
    sizes, K, C, L, loss, dt = SHAPES[case]
    rng = np.random.default_rng(9500 + CASES.index(case))
    hs = []
    for i, n in enumerate(sizes):
        g = _graph(rng, n, C, loss)
        if case == "bigcl" and i == 0:
            ids = rng.permutation(np.repeat(np.arange(2), (70, 5)))     # ids 2 .. 7 unused
        else:
            ids = rng.permutation(np.arange(n) % K)             # every cluster used, sizes within one of each other
        h = hetero_from_clusters(g, ids, K)
        if case == "novv" and i == 0:
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
    model.fronts_loss = loss                                    # (run_one_launch takes model and batch alone)
    return model, d, host


def check_structure(case, host):
    """The property of the host batch the case is named for."""
    from graph_hscn import engine
    sizes, K, C, L, loss, dt = SHAPES[case]
    n_local = np.diff(host["local"].ptr.numpy())
    n_virt = np.diff(host["virtual"].ptr.numpy())
    assert tuple(n_local) == sizes
    used = [2 if case == "bigcl" and i == 0 else min(K, n) for i, n in enumerate(sizes)]
    assert n_virt.tolist() == used
    if case in TILES:
        assert (int(n_local.max()) + 15) // 16 == TILES[case]
    ll = host.edge_index_dict[engine.LL]
    if case == "n1":
        assert ll.size(1) == 0
    else:
        assert int(np.bincount(ll[1].numpy()).max()) <= 6       # 16-byte row records
    if case == "n513_L2":
        assert int(n_local.max()) * (H // 4) > 8 * 256          # float4 words of a_1 beyond the loading waves' registers
    lv = host.edge_index_dict[engine.LV]
    members = np.bincount(lv[1].numpy(), minlength=int(n_virt.sum()))
    if case == "nv16":
        assert int(members.max()) <= 7
    if case == "bigcl":
        assert sorted(members[:2].tolist()) == [5, 70]
    if case == "novv":
        vv = host.edge_index_dict[engine.VV]
        assert not bool((vv < int(n_virt[0])).any()) and vv.size(1) > 0


@pytest.mark.parametrize("case", CASES)
def test_one_launch_step_phase1(case):
    from oracle import models as OM
    from tests.helpers import ATOL, grads_close, pool_order_close, scale_close
    from graph_hscn.step import ResidentTrainStep
    sizes, K, C, L, loss, dt = SHAPES[case]
    model, d, host = build_case(case)
    check_structure(case, host)
    pair = ResidentTrainStep(model, d, loss, one_launch=False)
    pair.run()
    one = run_one_launch(model, d)
    assert one.virtual is not None and one.idle_cus
    assert step_variant(one) == EXPECTED[case], "the case runs the launch form it is named for"
    assert torch.equal(one.virtual, pair.virtual)
    assert pool_order_close(one.pred, pair.pred) and pool_order_close(one.score, pair.score)
    assert grads_close(one.grads[:-1], pair.grads[:-1], rel=1e-5) and pool_order_close(one.grads[-1], pair.grads[-1])
    assert bool(torch.isfinite(one.grads).all()) and float(one.grads[:-1].abs().max()) > 0
    half = dt == "f16"
    store = OM.half_storage if half else (lambda t: t)
    ref = OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L)
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        x = {k: v.float() for k, v in host.x_dict.items()}
        kw = {"store": OM.half_storage} if half else {}
        want = ref(x, host.edge_index_dict, host["local"].batch, host.num_graphs, **kw)
        xo = {k: store(v) for k, v in x.items()}
        for conv in ref.convs:
            xo = {k: store(v.relu()) for k, v in conv(xo, host.edge_index_dict).items()}
    d_pred = float((one.pred.float().cpu() - want).abs().max())
    d_virt = float((one.virtual.float().cpu() - xo["virtual"]).abs().max())
    print(f"[{case_id(case)}] |pred - oracle| = {d_pred:.3e}  |virtual - oracle| = {d_virt:.3e} "
          f"(max |virtual| = {float(xo['virtual'].abs().max()):.3e})")
    if half:
        assert d_pred <= 2.0 ** -10 * max(1.0, float(want.abs().max()))
        assert scale_close(one.virtual.float(), xo["virtual"], rel=2.0 ** -10)
    else:
        assert d_pred <= ATOL
        assert scale_close(one.virtual, xo["virtual"])
    got = step_bits(one)
    with np.load(os.path.join(GOLDEN, f"step_bits_{case_id(case)}.npz")) as gold:
        assert sorted(gold.files) == sorted(got)
        for k in got:
            assert got[k].shape == gold[k].shape and got[k].tobytes() == gold[k].tobytes(), k


def test_replay():
    """Three launches in a row and one replay of a captured launch: the per-step epoch word advances, nothing else may."""
    from graph_hscn.step import ResidentTrainStep
    model, d, _ = build_case("tiles_257")
    one = ResidentTrainStep(model, d, "cross_entropy", one_launch=True)
    assert one.one_launch
    runs = []
    for _ in range(3):
        one.run()
        torch.cuda.synchronize()
        runs.append(step_bits(one))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.run()
    one.grads.zero_()
    one.pred.zero_()
    graph.replay()
    torch.cuda.synchronize()
    one.check()
    runs.append(step_bits(one))
    with np.load(os.path.join(GOLDEN, f"step_bits_{case_id('tiles_257')}.npz")) as gold:
        for r in runs:
            for k in r:
                assert r[k].tobytes() == runs[0][k].tobytes() == gold[k].tobytes(), k
