"""The one-launch step (csrc/resident_step.h) where the front of its local program and its head were rescheduled:

  * the local prologue stages only the edges in front of the structure build; features, layer weights, head weights and
    the target row wait in registers as raw loaded words and are parked in LDS BEHIND the build, where the zero padding
    is applied (with tail loops for n H > 8 RT words of features and for wide heads);
  * the fast head (H = 16, C <= 16) runs on two waves: one computes the gradient chain, the other recomputes
    pool -> z -> pred and owns the pred / score stores, the loss terms and the loss column; wider heads stay on one wave.

The cases also cover two reschedulings that were built, measured and taken out again: the head's
outer-product partials written by the last waves behind their row tiles of the first backward layer (hence the tile
counts around the wave count), and layer 0's attention logits of the virtual program computed beside its CSR builds
(hence the cluster-count and empty-relation cases).  Whoever tries either again has the fixtures.

All of it is scheduling: no sum and no rounding changes.  So every case is held

  * bit for bit to ``tests/golden/step_bits_fronts_<case>.npz``: prediction, score, every gradient, the loss and the
    final virtual features of the one-launch step of the commit BEFORE these changes on the same inputs on an MI355X
    (``tools/record_step_bits.py OUTDIR tests.test_gpu_step_fronts`` wrote them);
  * to the launch pair and to the CPU oracle with the bounds of tests/test_gpu_step_big_clusters.py (final virtual
    features bit for bit against the pair; prediction, score and loss by ``pool_order_close``; gradients by
    ``grads_close(rel=1e-5)``; the prediction within ATOL of the oracle's, the virtual features by ``scale_close``; half
    storage: the oracle emulates the rounding points and the bound is 2^-10 of the tensor's magnitude).

Cases (H = 16, F = 9; a batch of 3 - 4 graphs each; K = 8 clusters, C = 10, L = 3, cross-entropy, float storage unless
the case says otherwise):

  one_tile     n = 9, 12, 16, 13         one 16-row tile on a 4-wave workgroup: waves >= ntile idle; the loss wave
                                         (wave 1 of 4) owns no tile
  tiles_240    n = 240, 100, 17          15 tiles on 16 waves: the last wave owns none
  tiles_241    n = 241, 100, 17          16 tiles: the last wave owns one
  tiles_257    n = 257, 100, 17          17 tiles: wave 0 owns two
  over_520     n = 520, 17, 33; L = 2    outside StepLCaps / StepVCaps: run-time layouts; 520 x 16 > 8 x 1024 feature
                                         words, so the park's tail loop runs (L = 2: three layers of a 520-node graph
                                         are more than a CU's LDS holds, the step does not take them)
  hub          n = 100 (hub), 33, 17     a row of >= 7 edges: the general CSR build in front of the park
  C1 C16 C17   n = 70, 33, 17            fast head at its narrowest and widest, general head just above
  l1           n = 70, 33, 17            the other loss kind
  L1 L2        n = 257, 100, 17          L = 1: no hand-off; L = 2: one hand-off, in layer 0's neighbour
  f16          n = 257, 100, 17          half storage
  nv1          n = 40, 17, 64; K = 1     one virtual node, one softmax chunk (4-wave workgroups)
  nv16         n = 100, 70, 33; K = 16   16 clusters of <= 7 members: the DPP-row path of the cluster reduce
  novv         n = 100, 33, 17           the first graph has no virtual->virtual edge at all
  C16_4w       n = 40, 17, 64; C = 16    the widest fast head on a 4-wave workgroup: 560 head and target words on 256
                                         threads, so the head's tail loop (words past 2 RT) runs

Each case asserts the launch form it is named for (hscn_resident_launch_plan_ex through ``step_variant``) and, on the
host batch, the structural property it is named for (tile counts, the hub row, cluster counts, the empty relation)."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_step_layouts import step_bits, step_variant  # noqa: F401  (the recorder takes them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, F = 16, 9
# name -> (graph sizes, K, C, L, loss, storage type)
SHAPES = {
    "one_tile": ((9, 12, 16, 13), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_240": ((240, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_241": ((241, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "tiles_257": ((257, 100, 17), 8, 10, 3, "cross_entropy", "f32"),
    "over_520": ((520, 17, 33), 8, 10, 2, "cross_entropy", "f32"),
    "hub": ((100, 33, 17), 8, 10, 3, "cross_entropy", "f32"),
    "C1": ((70, 33, 17), 8, 1, 3, "cross_entropy", "f32"),
    "C16": ((70, 33, 17), 8, 16, 3, "cross_entropy", "f32"),
    "C17": ((70, 33, 17), 8, 17, 3, "cross_entropy", "f32"),
    "l1": ((70, 33, 17), 8, 10, 3, "l1", "f32"),
    "L1": ((257, 100, 17), 8, 10, 1, "cross_entropy", "f32"),
    "L2": ((257, 100, 17), 8, 10, 2, "cross_entropy", "f32"),
    "f16": ((257, 100, 17), 8, 10, 3, "cross_entropy", "f16"),
    "nv1": ((40, 17, 64), 1, 10, 3, "cross_entropy", "f32"),
    "nv16": ((100, 70, 33), 16, 10, 3, "cross_entropy", "f32"),
    "novv": ((100, 33, 17), 8, 10, 3, "cross_entropy", "f32"),
    "C16_4w": ((40, 17, 64), 8, 16, 3, "cross_entropy", "f32"),
}
CASES = list(SHAPES)

# The launch form of each case, from the planner's rules (csrc/resident_kernels.h, plan_step): 4-wave workgroups up to
# 64 nodes, else 16 waves; the virtual program's layout at compile time within StepVCaps (n <= 448, <= 32 clusters); the
# local program's beside it within StepLCaps (n <= 448, <= 1024 ll edges, L = 3, C <= 16).
EXPECTED = {name: dict(threads=1024, local_fixed=1, virtual_fixed=1) for name in CASES}
EXPECTED["one_tile"] = EXPECTED["nv1"] = EXPECTED["C16_4w"] = dict(threads=256, local_fixed=0, virtual_fixed=0)
EXPECTED["over_520"] = dict(threads=1024, local_fixed=0, virtual_fixed=0)
EXPECTED["C17"] = EXPECTED["L1"] = EXPECTED["L2"] = dict(threads=1024, local_fixed=0, virtual_fixed=1)


def case_id(case):
    return f"fronts_{case}"


def _graph(rng, n, C, loss, hub=False):
    """A chain with a chord every 5 nodes, both directions stored (rows of at most 6 edges); ``hub``: node 0 also
    receives an arc from 7 other nodes."""
    from graph_hscn.data import Data
    src = list(range(n - 1))
    dst = list(range(1, n))
    for a in range(0, n - 5, 5):
        src.append(a)
        dst.append(a + 4)
    e = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    e = np.concatenate([e, e[::-1]], 1)
    if hub:
        leaves = rng.choice(np.arange(6, n), size=7, replace=False)
        e = np.concatenate([e, np.stack([leaves, np.zeros(7, dtype=np.int64)])], 1)
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
    rng = np.random.default_rng(9000 + CASES.index(case))
    hs = []
    for i, n in enumerate(sizes):
        g = _graph(rng, n, C, loss, hub=(case == "hub" and i == 0))
        ids = rng.permutation(np.arange(n) % K)                 # every cluster used, sizes within one of each other
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


def run_one_launch(model, d):
    from graph_hscn.step import ResidentTrainStep
    one = ResidentTrainStep(model, d, model.fronts_loss, one_launch=True)
    assert one.one_launch
    one.run()
    one.run()                     # buffers are rewritten, not accumulated into
    torch.cuda.synchronize()
    one.check()
    return one


def check_structure(case, host):
    """The property of the host batch the case is named for."""
    from graph_hscn import engine
    sizes, K, C, L, loss, dt = SHAPES[case]
    n_local = np.diff(host["local"].ptr.numpy())
    n_virt = np.diff(host["virtual"].ptr.numpy())
    assert tuple(n_local) == sizes
    assert all(nv == min(K, n) for nv, n in zip(n_virt, sizes))
    tiles = (int(n_local.max()) + 15) // 16
    if case.startswith("tiles_") or case == "one_tile":
        assert tiles == {"one_tile": 1, "tiles_240": 15, "tiles_241": 16, "tiles_257": 17}[case]
    if case == "over_520":
        assert int(n_local.max()) * H > 8 * 1024
    ll = host.edge_index_dict[engine.LL]
    indeg = np.bincount(ll[1].numpy(), minlength=int(n_local.sum()))
    assert (int(indeg.max()) >= 7) == (case == "hub")           # every other graph: 16-byte row records (<= 6 edges)
    if case == "nv16":
        lv = host.edge_index_dict[engine.LV]
        assert int(np.bincount(lv[1].numpy()).max()) <= 16
    if case == "novv":
        vv = host.edge_index_dict[engine.VV]
        assert not bool((vv < int(n_virt[0])).any()) and vv.size(1) > 0


@pytest.mark.parametrize("case", CASES)
def test_one_launch_step_fronts(case):
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
