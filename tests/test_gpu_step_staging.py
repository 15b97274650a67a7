"""The one-launch step's input staging (csrc/resident_step.h prologue; the virtual program, csrc/resident_kernels.h
hscn_fwd_body modes 5 and 6, stages through registers and rides along) at the edges of its lane masks.

With float storage the local program sends features, transposed layer weights, head weights and the target row
straight from global memory into LDS (glds(): wave-linear destination, masked lanes write nothing) and zeroes the
padding words -- feature columns and layer-0 weight rows k >= F -- with plain LDS stores.  What can go wrong is a
word that neither path writes (it keeps what the previous workgroup on that CU left there), a word both write, or
a word read before it has landed; none of it shows on the workload's own shape (F = 9, n ~ 150).  The cases put the
masks on almost every lane (F = 1), on some (F = 9, 15) and on none (F = 16); n H on a wave boundary (n = 4), short of
it (3) and past it (5); n H around the 1024-thread stride (n = 63, 64, 65) and one word (n = 1); the cap of the fixed
layout (n = 444) and a graph beyond the prologue's fixed share of XPT RT = 8192 words (n = 513: the tail loop); 4-wave
batches; L = 1, 2, 3; C = 1, 10, 16, 17 (head words around a wave boundary: the fast head and the wide head); 1, 16
and 32 clusters; graphs without edges.  Only the route of the bytes differs between forms, so every case is held

  * bit for bit to ``tests/golden/step_bits_staging_<case>.npz``: what the one-launch step of the commit BEFORE the
    direct staging computed on the same inputs on an MI355X
    (``tools/record_step_bits.py OUTDIR tests.test_gpu_step_staging`` wrote them);
  * to the launch pair (whose programs keep the register route): final virtual features bit for bit;
  * to the CPU oracle with the bounds of tests/test_gpu_step_big_clusters.py: the prediction within ATOL, the final
    virtual features by ``scale_close``.

``test_padding_is_rewritten`` runs the F = 16 batch and then the F = 1 batch of the same sizes: a padding word that
is not zeroed then holds a feature of the first batch."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_step_layouts import run_one_launch, step_bits, step_variant  # noqa: F401  (the recorder takes them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = 16
# graphs of a batch: (nodes, clusters, has edges)
BATCHES = {
    "waves": ((3, 1, True), (4, 1, True), (5, 1, True), (4, 1, False)),
    "stride": ((1, 1, True), (63, 16, True), (64, 32, True), (65, 32, True)),
    "small": ((63, 16, True), (64, 32, True), (33, 1, False), (1, 1, True)),
    "cap": ((444, 32, True), (64, 16, True)),
    "tail": ((513, 16, True), (5, 1, True)),
    "pad": ((65, 16, True), (64, 1, True), (5, 1, True)),
}
# (batch, F, L, C)
CASES = [("waves", 9, 3, 10), ("stride", 15, 2, 16), ("small", 1, 1, 1), ("cap", 16, 3, 17), ("cap", 9, 3, 10),
         ("tail", 9, 2, 10), ("pad", 16, 3, 10), ("pad", 1, 3, 10)]
# threads per workgroup the host plans for the batch: 4 waves up to 64 nodes, 16 beyond
THREADS = {"waves": 256, "small": 256, "stride": 1024, "cap": 1024, "tail": 1024, "pad": 1024}


def case_id(case):
    b, F, L, C = case
    return f"staging_{b}_F{F}_L{L}_C{C}"


def _graph(rng, n, F, C, edges):
    """A chain with a chord every 16 nodes, both directions stored (molecule-like rows), or no edge at all."""
    from graph_hscn.data import Data
    src = list(range(n - 1)) if edges else []
    dst = list(range(1, n)) if edges else []
    for a in range(0, n - 7 if edges else 0, 16):
        src.append(a)
        dst.append(a + 6)
    e = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    e = np.concatenate([e, e[::-1]], 1)
    e = e[:, rng.permutation(e.shape[1])]                       # edge order is part of the result: fix an arbitrary one
    x = torch.from_numpy((rng.integers(1, 5, (n, F)) / 4.0).astype(np.float32))     # no zero: a stale word shows
    y = torch.from_numpy((rng.random((1, C)) < 0.4).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(np.ascontiguousarray(e)), y=y, num_nodes=n)


def build_case(case, dev="cuda:0"):
    """-> (model, device batch, host batch); deterministic in ``case`` alone."""
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.model.hscn import HSCN
    name, F, L, C = case
    rng = np.random.default_rng(9000 + 100 * sorted(BATCHES).index(name) + 10 * L + F)
    hs = []
    for n, nv, edges in BATCHES[name]:
        g = _graph(rng, n, F, C, edges)
        hs.append(hetero_from_clusters(g, rng.permutation(np.arange(n) % nv), 32))
    host = HeteroBatch.from_data_list(hs)
    d = host.to(dev)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.from_numpy((0.3 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    model = model.to(dev)
    model.compute_virtual = True
    return model, d, host


def _check(case, one, pair, model, host):
    from oracle import models as OM
    from tests.helpers import ATOL, scale_close
    name, F, L, C = case
    assert one.virtual is not None and one.idle_cus
    assert step_variant(one)["threads"] == THREADS[name], "the case runs the workgroup size it is named for"
    got = step_bits(one)
    with np.load(os.path.join(GOLDEN, f"step_bits_{case_id(case)}.npz")) as gold:
        assert sorted(gold.files) == sorted(got)
        for k in got:
            assert got[k].shape == gold[k].shape and got[k].tobytes() == gold[k].tobytes(), k
    assert torch.equal(one.virtual, pair.virtual)
    ref = OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L)
    ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        x = {k: v.float() for k, v in host.x_dict.items()}
        want = ref(x, host.edge_index_dict, host["local"].batch, host.num_graphs)
        xo = x
        for conv in ref.convs:
            xo = {k: v.relu() for k, v in conv(xo, host.edge_index_dict).items()}
    d_pred = float((one.pred.float().cpu() - want).abs().max())
    d_virt = float((one.virtual.float().cpu() - xo["virtual"]).abs().max())
    print(f"[{case_id(case)}] |pred - oracle| = {d_pred:.3e}  |virtual - oracle| = {d_virt:.3e} "
          f"(max |virtual| = {float(xo['virtual'].abs().max()):.3e})")
    assert d_pred <= ATOL
    assert scale_close(one.virtual, xo["virtual"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_launch_step_staging(case):
    from graph_hscn.step import ResidentTrainStep
    model, d, host = build_case(case)
    pair = ResidentTrainStep(model, d, "cross_entropy", one_launch=False)
    pair.run()
    one = run_one_launch(model, d)
    _check(case, one, pair, model, host)


def test_padding_is_rewritten():
    """F = 16 first (every word of A[0] and of layer 0's weight rows is a non-zero feature or a weight), F = 1 second
    on the same device: the F = 1 step must not see what the first left in its padding words."""
    from graph_hscn.step import ResidentTrainStep
    first, second = ("pad", 16, 3, 10), ("pad", 1, 3, 10)
    m1, d1, _ = build_case(first)
    for _ in range(4):                       # (on as many CUs as the second batch's workgroups may land on)
        run_one_launch(m1, d1)
    model, d, host = build_case(second)
    one = run_one_launch(model, d)
    pair = ResidentTrainStep(model, d, "cross_entropy", one_launch=False)
    pair.run()
    _check(second, one, pair, model, host)
