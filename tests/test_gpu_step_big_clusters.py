"""The virtual program's cluster reduce (csrc/resident_kernels.h, reduce_virtual, chunk path) on clusters of more than
64 members, through the one-launch step and the launch pair.

A cluster of more than 64 members is cut into 64-member chunks, one wave each; every chunk wave needs the whole
cluster's softmax max and denominator.  Up to ceil(StepVCaps::N / 64) = 7 logits per lane are read once and kept in
registers, larger clusters walk the cluster twice; the last arriver of a cluster folds the chunks' partial rows in chunk
order and applies the two 16 x 16 transforms from registers; chunks are drawn from an LDS counter by whichever wave is
free (12 waves of a 16-wave workgroup enter the reduce, 3 of a 4-wave one, the loading waves join later).  None of
these forms changes a sum or its order, so every case is held

  * to the launch pair: final virtual features bit for bit; prediction, score, loss and gradients with the bounds
    tests/test_gpu_step_layouts.py uses;
  * to the CPU oracle: the prediction within ATOL, the final virtual features by ``scale_close`` (obtained as
    tests/test_gpu_full_size.py does: the oracle's layers applied with a ReLU after each).  Half storage: the rounding
    points are part of the function, so the oracle emulates them (oracle.models.half_storage after the input and after
    every layer) and the bound is 2^-10 of the tensor's magnitude, one ulp of the storage type, as
    tests/test_gpu_full_size.py and tests/test_gpu_f16.py use;
  * bit for bit to ``tests/golden/step_bits_bigcl_<case>.npz``: what the one-launch step of the commit BEFORE the
    register form of the logits and the register finisher computed on the same inputs on an MI355X
    (``tools/record_step_bits.py OUTDIR tests.test_gpu_step_big_clusters`` wrote them).

Graphs (n: cluster member counts), K = 8, H = 16, F = 9:

  fixed (16 waves, compile-time layouts at L = 3; every graph has fewer chunks than entering waves)
      320: 64, 128, 128     chunk boundaries
      330: 65, 257, 8       5 chunks of one cluster, a one-member tail chunk
      200: 129, 71          two and three chunks
       17: 17               a single chunk
      444: 444              7 registers per lane: the top of the register form
  over  (max_n just above StepVCaps::N: run-time layout)
      449: 449              more members than the registers hold: the two loops
       17: 17
  many  (16 waves)
      444: 6 x 65, 54       13 chunks on the 12 waves that enter the reduce: a second round
      320: 64, 128, 128
  small (4-wave workgroups: 3 waves enter the reduce)
       17: 17               one chunk, two idle waves
       64: 17, 17, 15, 15   4 chunks on 3 waves: a second round

Members of a cluster are scattered over the graph (a seeded permutation), so a chunk's members are no contiguous rows."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_step_layouts import run_one_launch, step_bits, step_variant  # noqa: F401  (the recorder takes them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, K, C, F = 16, 8, 10, 9
BATCHES = {
    "fixed": ((320, (64, 128, 128)), (330, (65, 257, 8)), (200, (129, 71)), (17, (17,)), (444, (444,))),
    "over": ((449, (449,)), (17, (17,))),
    "many": ((444, (65, 65, 65, 65, 65, 65, 54)), (320, (64, 128, 128))),
    "small": ((17, (17,)), (64, (17, 17, 15, 15))),
}
# What each batch is named for, found with the host query (hscn_resident_launch_plan_ex on the batch's maxima): threads
# per workgroup; the virtual program's layout at compile time for 16-wave workgroups up to StepVCaps::N = 448 nodes, the
# local program's beside it at L = 3 (StepLCaps::L; these graphs have at most 942 <= StepLCaps::ELL edges).
def expected_variant(name, L):
    if name == "small":
        return dict(threads=256, local_fixed=0, virtual_fixed=0)
    if name == "over":
        return dict(threads=1024, local_fixed=0, virtual_fixed=0)
    return dict(threads=1024, local_fixed=int(L == 3), virtual_fixed=1)


# (batch, L, storage type)
CASES = [("fixed", 3, "f32"), ("fixed", 2, "f32"), ("fixed", 3, "f16"), ("over", 3, "f32"), ("over", 2, "f32"),
         ("many", 3, "f32"), ("many", 2, "f32"), ("small", 3, "f32")]


def case_id(case):
    b, L, dt = case
    return f"bigcl_{b}_L{L}_{dt}"


def _graph(rng, n):
    """A chain with a chord every 16 nodes, both directions stored: molecule-like rows (at most 4 edges), at most
    2.2 n <= 1024 edges at n = 444 (inside StepLCaps)."""
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
    y = torch.from_numpy((rng.random((1, C)) < 0.4).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=y, num_nodes=n)


def _ids(rng, n, counts):
    assert sum(counts) == n and len(counts) <= K
    return rng.permutation(np.repeat(np.arange(len(counts)), counts))


def build_case(case, dev="cuda:0"):
    """-> (model, device batch, host batch); deterministic in ``case`` alone."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.model.hscn import HSCN
    name, L, dt = case
    rng = np.random.default_rng(7000 + 10 * L + sorted(BATCHES).index(name))
    hs = []
    for n, counts in BATCHES[name]:
        g = _graph(rng, n)
        hs.append(hetero_from_clusters(g, _ids(rng, n, counts), K))
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


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_launch_step_big_clusters(case):
    from oracle import models as OM
    from tests.helpers import ATOL, grads_close, pool_order_close, scale_close
    from graph_hscn.step import ResidentTrainStep
    name, L, dt = case
    model, d, host = build_case(case)
    pair = ResidentTrainStep(model, d, "cross_entropy", one_launch=False)
    pair.run()
    one = run_one_launch(model, d)
    assert one.virtual is not None and one.idle_cus
    assert step_variant(one) == expected_variant(name, L), "the case runs the layout form it is named for"
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
