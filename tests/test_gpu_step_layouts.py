"""The one-launch step (csrc/resident_step.h) at the edges of its local program's LDS layout forms.

A batch of 16-wave workgroups at H = 16, L = 3, C <= 16 inside StepLCaps (n <= 448, <= 1024 ll edges per graph) runs
the local program with its LDS layout fixed at compile time; every other batch the run-time layout compiled in beside
it; graphs of at most 64 nodes the 4-wave form.  In all of them layer 0's weight gradient reads the features where
the prologue parked them in LDS (the wave-private transposition scratch of the one-phase backward lives in the
partial-tile buffer / in A[L]).  None of that changes a sum or its order, so every case is held

  * to the launch pair, with the bounds tests/test_gpu_step.py uses for the one-launch step (final virtual features
    bit for bit; prediction, score and loss by ``pool_order_close``; gradients by ``grads_close(rel=1e-5)``), and the
    float prediction to the CPU oracle's within ATOL;
  * bit for bit to ``tests/golden/step_bits_<case>.npz``: what the one-launch step of the commit BEFORE these layout
    forms computed on the same inputs on an MI355X (tools/record_step_bits.py wrote them).

Graph sizes: 1, 15, 16, 17, 33 (tile edges of the 16-row tiles) and 257 (17 tiles: two rounds on 16 waves); one graph
carries a row of 7 edges (general CSR build and CSR walk; the others are molecule-like: 16-byte row records), one a
directed ll relation.  Inputs and weights come from numpy generators: nothing depends on a library's initialiser."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, K, C = 16, 8, 10
SIZES = {"small": (1, 15, 16, 17, 33),            # max_n <= 64: 4-wave workgroups, run-time layout
         "mixed": (1, 15, 16, 17, 33, 257),       # 16 waves; L = 3: the compile-time layout
         "over": (17, 449)}                       # max_n just above StepLCaps::N = 448: run-time layout, 16 waves

# (batch, L, F, virtual branch, storage type)
CASES = ([("mixed", L, F, v, "f32") for L in (1, 2, 3) for F in (9, 16) for v in (True, False)]
         + [("mixed", 3, 9, True, "f16"), ("mixed", 3, 16, False, "f16"), ("mixed", 2, 9, True, "f16")]
         + [("small", 1, 9, True, "f32"), ("small", 2, 16, False, "f32"), ("small", 3, 9, True, "f32"),
            ("small", 3, 16, False, "f32"), ("small", 3, 9, True, "f16")]
         + [("over", 3, 9, True, "f32"), ("over", 3, 16, False, "f32"), ("over", 3, 9, True, "f16")])


# What each batch is named for, found with the host query (hscn_resident_launch_plan_ex; SIZES' maxima with K = 8 and
# these graphs' edge counts): threads per workgroup, and whether the local / the virtual program takes its LDS layout at
# compile time -- the local one at L = 3 only (StepLCaps::L), and with a virtual job only beside a fixed virtual program.
def expected_variant(name, L, virt):
    return {"small": dict(threads=256, local_fixed=0, virtual_fixed=0),
            "mixed": dict(threads=1024, local_fixed=int(L == 3), virtual_fixed=int(virt)),
            "over": dict(threads=1024, local_fixed=0, virtual_fixed=0)}[name]


def step_variant(one):
    """The instantiation ``one``'s launch takes, asked of the library for the batch's maxima."""
    from graph_hscn import _hip
    N, V, F, H, L, C, B = one.dims
    m = one.meta
    with_job = bool(one.idle_cus and one.virtual is not None)
    plan = _hip.resident_launch_plan(F, H, L, C, m.max_n, m.max_v, m.max_ell, m.max_evv,
                                     launch="step_virtual" if with_job else "step")
    assert plan is not None, "the one-launch step takes this batch"
    return {k: plan[k] for k in ("threads", "local_fixed", "virtual_fixed")}


def case_id(case):
    b, L, F, v, dt = case
    return f"{b}_L{L}_F{F}_{'virt' if v else 'novirt'}_{dt}"


def _graph(rng, n, F, hub=False, directed=False):
    """A chain with a few chords (every row of at most 6 edges, both directions stored) -- or, ``directed``, forward
    arcs only; ``hub``: node 0 also receives an arc from 7 other nodes (a row of >= 7 edges)."""
    from graph_hscn.data import Data
    src = list(range(n - 1))
    dst = list(range(1, n))
    for a in range(0, n - 5, 5):
        src.append(a)
        dst.append(a + 4)
    e = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    if not directed:
        e = np.concatenate([e, e[::-1]], 1)
    if hub:
        leaves = rng.choice(np.arange(6, n), size=7, replace=False)
        e = np.concatenate([e, np.stack([leaves, np.zeros(7, dtype=np.int64)])], 1)
    e = e[:, rng.permutation(e.shape[1])]                       # edge order is part of the result: fix an arbitrary one
    x = torch.from_numpy((rng.integers(0, 5, (n, F)) / 4.0).astype(np.float32))     # exact in half storage
    y = torch.from_numpy((rng.random((1, C)) < 0.4).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=y, num_nodes=n)


def build_case(case, dev="cuda:0"):
    """-> (model, device batch, host batch); deterministic in ``case`` alone."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.model.hscn import HSCN
    name, L, F, virt, dt = case
    rng = np.random.default_rng(1000 * L + F)
    graphs = [_graph(rng, n, F, hub=(n == 33 or n == 449), directed=(n == 17)) for n in SIZES[name]]
    host = HeteroBatch.from_data_list([hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs])
    d = host.to(dev)
    if dt == "f16":
        d = d.with_feature_dtype(torch.float16)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.from_numpy((0.3 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    model = model.to(dev)
    model.compute_virtual = virt
    return model, d, host


def run_one_launch(model, d):
    from graph_hscn.step import ResidentTrainStep
    one = ResidentTrainStep(model, d, "cross_entropy", one_launch=True)
    assert one.one_launch
    one.run()
    one.run()                     # buffers are rewritten, not accumulated into
    torch.cuda.synchronize()
    one.check()
    return one


def step_bits(one):
    """What the fixture holds of a step: float32 copies of everything it computed."""
    out = {"pred": one.pred, "score": one.score, "grads": one.grads}      # (grads[-1] = the loss)
    if one.virtual is not None:
        out["virtual"] = one.virtual
    return {k: v.detach().float().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_launch_step_layout_forms(case):
    from oracle import models as OM
    from tests.helpers import ATOL, grads_close, pool_order_close
    from graph_hscn.step import ResidentTrainStep
    name, L, F, virt, dt = case
    model, d, host = build_case(case)
    pair = ResidentTrainStep(model, d, "cross_entropy", one_launch=False)
    pair.run()
    one = run_one_launch(model, d)
    assert (one.virtual is not None) == virt
    assert step_variant(one) == expected_variant(name, L, virt), "the case runs the layout form it is named for"
    if virt:
        assert one.idle_cus                                   # the virtual branch rides on its own workgroups
        assert torch.equal(one.virtual, pair.virtual)
    assert pool_order_close(one.pred, pair.pred) and pool_order_close(one.score, pair.score)
    assert grads_close(one.grads[:-1], pair.grads[:-1], rel=1e-5) and pool_order_close(one.grads[-1], pair.grads[-1])
    assert bool(torch.isfinite(one.grads).all()) and float(one.grads[:-1].abs().max()) > 0
    if dt == "f32":
        ref = OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L)
        ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            want = ref({k: v.float() for k, v in host.x_dict.items()}, host.edge_index_dict, host["local"].batch,
                       host.num_graphs)
        assert torch.allclose(one.pred.cpu(), want, atol=ATOL, rtol=1e-5), float((one.pred.cpu() - want).abs().max())
    got = step_bits(one)
    with np.load(os.path.join(GOLDEN, f"step_bits_{case_id(case)}.npz")) as gold:
        assert sorted(gold.files) == sorted(got)
        for k in got:
            assert got[k].shape == gold[k].shape and got[k].tobytes() == gold[k].tobytes(), k
