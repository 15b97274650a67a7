"""DMoN pooling without a GPU: the oracle restatement (tests/dmon_oracle.py) against autograd and closed forms, the
bar the GPU tests apply tried on a further float32 draw, the SCN keyword's refusals, and the C entry points'
argument checks (the built library alone: every refusal precedes the first launch)."""
import ctypes

import pytest
import torch

from tests import dmon_oracle as DO


@pytest.mark.parametrize("K", [2, 5])
def test_hand_gradient_equals_float64_autograd(K):
    graphs = DO.case(K, 3, sizes=[1, 2, 37, 70])
    hand, auto = DO.backward(graphs), DO.autograd_backward(graphs)
    assert float(hand.abs().max()) > 1e-3
    assert float((hand - auto).abs().max()) <= 1e-13 * max(1.0, float(auto.abs().max()))
    # each left-out term changes the gradient (the one-directional edges are what tells A^T from A)
    for variant in ({"null": False}, {"at_half": False}, {"cluster": False}):
        assert float((DO.backward(graphs, **variant) - hand).abs().max()) > 1e-6, variant


def test_one_cluster_is_a_fixed_point():
    graphs = DO.case(1, 0, sizes=[1, 2, 37])
    f = DO.forward(graphs)
    assert float(f["spectral"].abs()) <= 1e-15 and float(f["cluster"].abs()) <= 1e-15
    assert float(DO.backward(graphs).abs().max()) == 0.0
    assert float(DO.autograd_backward(graphs).abs().max()) == 0.0


@pytest.mark.parametrize("c", [3, 8])
def test_two_cliques_closed_form(c):
    """Two cliques of c nodes, self loops included, split exactly (logits +-30, K = 2): every edge is inside a cluster,
    so tr(S^T A S) = 2m = 2 c^2, d^T S = (c^2, c^2) and the null term is 2 c^4 / 2m = c^2 = m: spectral = -(2m - m) / 2m
    = -0.5; S^T S = c I gives ortho = 0; the cluster sizes (c, c) give |c| sqrt(2) / 2c - 1 = 0."""
    block = torch.cartesian_prod(torch.arange(c), torch.arange(c)).t()
    ei = torch.cat([block, block + c], 1)
    logits = torch.full((2 * c, 2), -30.0, dtype=torch.float64)
    logits[:c, 0] = 30.0
    logits[c:, 1] = 30.0
    f = DO.forward([(logits, torch.zeros(2 * c, 0), ei)])
    assert abs(float(f["spectral"]) + 0.5) <= 1e-14
    assert abs(float(f["ortho"])) <= 1e-14
    assert abs(float(f["cluster"])) <= 1e-14


def test_edgeless_graph_gives_zero_not_nan():
    g = torch.Generator().manual_seed(5)
    lone = (torch.randn(6, 3, generator=g, dtype=torch.float64), torch.zeros(6, 0), torch.zeros(2, 0, dtype=torch.long))
    f = DO.forward([lone])
    assert float(f["spectral"]) == 0.0 and float(f["two_m"][0]) == 0.0
    assert all(bool(torch.isfinite(f[k]).all()) for k in ("spectral", "ortho", "cluster", "S", "ss", "vec"))
    only_spectral = DO.backward([lone], weights=(1.0, 0.0, 0.0))
    assert float(only_spectral.abs().max()) == 0.0
    assert bool(torch.isfinite(DO.backward([lone])).all())
    assert float((DO.backward([lone]) - DO.autograd_backward([lone])).abs().max()) <= 1e-15


@pytest.mark.parametrize("K", [1, 2, 5, 64])
def test_the_gpu_bar_admits_a_further_float32_draw_and_keeps_its_teeth(K):
    """The inputs and the bar of tests/test_gpu_dmon.py::test_operator_against_the_float64_referee with a ninth
    relabelled float32 oracle evaluation in the kernel's place: a correct float32 evaluation passes (the ratios are
    printed), and against each one-term-short oracle the same evaluation is rejected."""
    graphs = DO.case(K, 7)
    ninth = DO.draws32(graphs, 1, first_seed=99)[0]
    assert DO.referee_case(ninth, graphs, f"ninth draw K={K}") <= 1.0


def test_scn_pool_keyword_refusals():
    from graph_hscn.model.hscn import SCN
    with pytest.raises(ValueError, match="kmeans"):
        SCN([16], "relu", 9, 4, pool="kmeans")
    for kw, K in ((dict(mincut_route="dense"), 4), (dict(mincut_route="auto"), 64)):
        with pytest.raises(ValueError, match="DMoN.*dense route"):
            SCN([16], "relu", 9, K, pool="dmon", **kw)
    assert SCN([16], "relu", 9, 4).pool == "mincut"
    m = SCN([16], "relu", 9, 4, pool="dmon", mincut_route="auto")      # auto below 64 clusters is the sparse route
    assert m.pool == "dmon" and not m._dense()
    assert m.resident_ok(None) is False                                # answered before the data is looked at


def test_pack_loss_grads_takes_a_third_slot():
    from graph_hscn.nn.functional import _pack_loss_grads
    a, b, c = torch.tensor(1.5), torch.tensor(-2.0), torch.tensor(0.25)
    assert _pack_loss_grads(a, b, "cpu").tolist() == [1.5, -2.0]
    assert _pack_loss_grads(None, b, "cpu").tolist() == [0.0, -2.0]
    assert _pack_loss_grads(None, None, "cpu").tolist() == [0.0, 0.0]
    assert _pack_loss_grads(a, None, "cpu", c).tolist() == [1.5, 0.0, 0.25]
    assert _pack_loss_grads(None, None, "cpu", None).tolist() == [0.0, 0.0, 0.0]


# a pointer that is never followed: every call below is refused before its first launch
_HERE = ctypes.addressof(ctypes.create_string_buffer(64))
_FWD = ["logits", "x", "rowptr", "col", "node_ptr", "S", "stats", "ss", "vec", "pooled_x", "pooled_adj", "losses",
        "num_nodes", "num_graphs", "K", "Fx", "stream"]
_BWD = ["S", "stats", "ss", "vec", "rowptr", "col", "rowptr_t", "col_t", "node_ptr", "g_losses", "g_logits",
        "num_nodes", "num_graphs", "K", "stream"]
_FWD_PTRS = ("logits", "rowptr", "col", "node_ptr", "S", "stats", "ss", "vec", "losses")
_BWD_PTRS = ("S", "stats", "ss", "vec", "rowptr", "col", "rowptr_t", "col_t", "node_ptr", "g_losses", "g_logits")


def _call(name, names, **kw):
    from graph_hscn import _hip
    sig = _hip._SIGNATURES[name][1]
    assert len(sig) == len(names)
    args = [None if t is ctypes.c_void_p else 0 for t in sig]
    for k, v in kw.items():
        args[names.index(k)] = v
    return getattr(_hip.lib(), name)(*args)


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    fwd = dict.fromkeys(_FWD_PTRS, _HERE)
    bwd = dict.fromkeys(_BWD_PTRS, _HERE)
    for name, names, ok, ptrs in (("hscn_dmon_sparse_fwd", _FWD, fwd, _FWD_PTRS),
                                  ("hscn_dmon_sparse_bwd", _BWD, bwd, _BWD_PTRS)):
        assert _call(name, names, **ok, num_graphs=1, K=0) == -1                       # HSCN_E_BADARG
        assert _call(name, names, **ok, num_graphs=1, K=257) == -1
        assert _call(name, names, **ok, num_graphs=0, K=8) == -1
        assert _call(name, names, **ok, num_graphs=1, K=8, num_nodes=-1) == -1
        assert _call(name, names, num_graphs=1, K=8) == -1                             # every pointer NULL
        for p in ptrs:                                                                 # each required pointer alone
            assert _call(name, names, **dict(ok, **{p: None}), num_graphs=1, K=8) == -1, (name, p)
        assert _call(name, names, num_graphs=1, K=256) == -1                           # NULL beats the LDS answer
        assert _call(name, names, **ok, num_graphs=1, K=256) == -3                     # HSCN_E_UNSUPPORTED
    assert _call("hscn_dmon_sparse_fwd", _FWD, **fwd, num_graphs=1, K=8, Fx=-1) == -1
    # the widest K a CU's 160 KB holds (include/hscn.h: forward (2 K^2 + 35 K + 20) * 4 bytes without x, backward
    # (K^2 + 34 K + 20) * 4) is refused one past it
    assert (2 * 134 * 134 + 35 * 134 + 20) * 4 <= 160 * 1024 < (2 * 135 * 135 + 35 * 135 + 20) * 4
    assert _call("hscn_dmon_sparse_fwd", _FWD, **fwd, num_graphs=1, K=135) == -3
    assert (186 * 186 + 34 * 186 + 20) * 4 <= 160 * 1024 < (187 * 187 + 34 * 187 + 20) * 4
    assert _call("hscn_dmon_sparse_bwd", _BWD, **bwd, num_graphs=1, K=187) == -3


def test_dmon_is_exported_beside_mincut():
    import graph_hscn.nn as nn_
    assert "dmon_pool_sparse" in nn_.__all__ and callable(nn_.dmon_pool_sparse)
    from graph_hscn.nn.functional import DMoNSparseFn   # noqa: F401
