"""Node-level tasks, host side: config fields, loaders, the node-labelled synthetic shape, the CPU restatement of the
weighted criterion, the node head's envelope, the refusals of the resident engines and the argument checks of the new
entry points.  CPU only: nothing here launches."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _hscn(task_level="node", vl=None, H=16, C=10):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, H, C, 3, vl_conv=vl, task_level=task_level)


def _mpnn(task_level="node"):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    return MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 10, 3, task_level=task_level)


def test_config_fields_default_to_graph_and_reach_the_builders():
    from graph_hscn.config.config import HSCNConfig, MPNNConfig
    from graph_hscn.model.hscn import build_hscn
    from graph_hscn.model.mpnn import build_mpnn
    assert HSCNConfig("relu").task_level == "graph" and MPNNConfig("gcn", "relu").task_level == "graph"
    assert build_hscn(HSCNConfig("relu"), 9, 10).task_level == "graph"
    assert build_mpnn(MPNNConfig("gcn", "relu"), 9, 10).task_level == "graph"
    m = build_hscn(HSCNConfig("relu", task_level="node"), 9, 10)
    assert m.task_level == "node" and m.node_head is not None
    assert build_mpnn(MPNNConfig("gcn", "relu", task_level="node"), 9, 10).task_level == "node"
    assert sorted(m.state_dict()) == sorted(build_hscn(HSCNConfig("relu"), 9, 10).state_dict())     # lin_1 / lin_2
    for bad in (lambda: HSCNConfig("relu", task_level="edge"), lambda: MPNNConfig("gcn", "relu", task_level="edge"),
                lambda: _hscn("edge"), lambda: _mpnn("edge")):
        with pytest.raises(ValueError):
            bad()


def test_node_labelled_shape_is_seeded_and_skewed():
    from graph_hscn.loader.synthetic import NODE_SHAPES, SHAPES, make_dataset
    assert "pascalvoc_sp_node" in NODE_SHAPES and "pascalvoc_sp_node" not in SHAPES
    a, b = make_dataset("pascalvoc_sp_node", 2, seed=3), make_dataset("pascalvoc_sp_node", 2, seed=3)
    plain = make_dataset("pascalvoc_sp", 2, seed=3)
    for g, h, p in zip(a, b, plain):
        assert torch.equal(g.y, h.y) and torch.equal(g.x, h.x) and torch.equal(g.edge_index, h.edge_index)
        assert g.y.dtype == torch.int64 and g.y.shape == (g.num_nodes,)
        assert 395 <= g.num_nodes <= 500 and g.x.shape == (g.num_nodes, 14)
        assert int(g.y.min()) >= 0 and int(g.y.max()) < 21
        assert p.y.shape == (1, 21)                                                    # the graph-level shape is as it was
    counts = torch.bincount(torch.cat([g.y for g in a]), minlength=21)
    assert int((counts == 0).sum()) >= 1                                               # a class absent at 2 graphs
    assert int(counts[0]) > 4 * int(counts[5]) > 0                                     # skewed


def test_loaders_accept_node_level_and_keep_per_node_labels():
    from graph_hscn.config.config import DataConfig, HSCNConfig
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import generate_hetero_data, hetero_loaders
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("pascalvoc_sp_node", 6, seed=1)
    rng = np.random.default_rng(0)
    clusters = [rng.integers(0, 4, g.num_nodes) for g in graphs]
    split = {"train": torch.tensor([0, 1, 2, 3]), "val": torch.tensor([4]), "test": torch.tensor([5])}
    cfg = DataConfig("pascalvoc_sp", batch_size=2, num_workers=0, task_level="node")
    assert cfg.task_level == "node"
    hs = generate_hetero_data(clusters, graphs, split, cfg, HSCNConfig("relu", num_clusters=4))
    for g, h in zip(graphs, hs):
        assert torch.equal(h["local"].y, g.y)
    loaders = hetero_loaders(cfg, hs, split)
    batch = next(iter(loaders[1]))
    assert torch.equal(batch["local"].y, graphs[4].y)
    hb = HeteroBatch.from_data_list(hs[:2])
    assert torch.equal(hb["local"].y, torch.cat([graphs[0].y, graphs[1].y]))
    cfg.task_level = "edge"
    with pytest.raises(NotImplementedError):
        generate_hetero_data(clusters, graphs, split, cfg, HSCNConfig("relu", num_clusters=4))
    with pytest.raises(NotImplementedError):
        hetero_loaders(cfg, hs, split)


@pytest.mark.parametrize("ignore", [None, -100, 2])
def test_cpu_weighted_criterion_is_cross_entropy_with_the_lrgb_weights_by_hand(ignore):
    from graph_hscn.loss import batch_class_weights, criterion
    g = torch.Generator().manual_seed(0)
    R, C = 200, 7
    pred = torch.randn(R, C, generator=g, dtype=torch.float64)
    true = torch.randint(0, C - 1, (R,), generator=g)                                  # class C - 1 is absent
    if ignore is not None:
        true[torch.rand(R, generator=g) < 0.3] = ignore
    kept = true if ignore is None else true[true != ignore]
    V = kept.numel()
    w = torch.zeros(C)
    for c in range(C):                                                                 # LRGB's rule, written out
        n_c = int((kept == c).sum())
        w[c] = (torch.tensor(V - n_c).float() / V) if n_c > 0 else 0.0
    assert float(w[C - 1]) == 0.0 and torch.equal(batch_class_weights(true, C, ignore), w)
    want = F.cross_entropy(pred, true, weight=w.double(), ignore_index=-100 if ignore is None else ignore)
    kw = {} if ignore is None else {"ignore_index": ignore}
    loss, score = criterion("weighted_cross_entropy", pred, true, **kw)
    assert torch.equal(loss, want) and torch.equal(score, F.log_softmax(pred, -1))
    loss2, _ = criterion("cross_entropy", pred, true, class_weight="batch", **kw)
    assert torch.equal(loss2, want)
    given = torch.rand(C, generator=g) + 0.5
    loss3, _ = criterion("cross_entropy", pred, true, class_weight=given, **kw)
    assert torch.equal(loss3, F.cross_entropy(pred, true, weight=given.double(),
                                              ignore_index=-100 if ignore is None else ignore))
    with pytest.raises(ValueError):
        criterion("cross_entropy", pred, F.one_hot(true.clamp_min(0), C).double(), class_weight="batch")
    with pytest.raises(ValueError):
        criterion("cross_entropy", pred, true, class_weight="sqrt")
    # neither keyword: the path as it was
    plain, _ = criterion("cross_entropy", pred, true.clamp_min(0))
    assert torch.equal(plain, F.nll_loss(F.log_softmax(pred, -1), true.clamp_min(0)))


def test_node_head_envelope_at_its_edges():
    from graph_hscn import _hip
    L = _hip.lib()
    for H, ok in ((8, 0), (16, 1), (32, 1), (64, 1), (128, 0), (24, 0)):
        assert L.hscn_node_head_supported(H, 10) == ok
    for C, ok in ((0, 0), (1, 1), (64, 1), (65, 0)):
        for H in (16, 64):
            assert L.hscn_node_head_supported(H, C) == ok
    assert L.hscn_node_head_rows_per_workgroup() == 256
    assert L.hscn_node_head_workspace_bytes(1000, 16, 10) == 4 * 26 * 17 * 4
    assert L.hscn_node_head_workspace_bytes(1000, 8, 10) == 0 and L.hscn_node_head_workspace_bytes(0, 16, 10) == 0
    assert L.hscn_node_head_workspace_bytes(1 << 40, 64, 64) == 0


def test_node_level_models_name_the_head_and_the_resident_engines_refuse():
    from graph_hscn.train import batching
    for m in (_hscn(), _hscn(vl="GAT"), _mpnn()):
        assert "node-level head" in m.resident_reason()
        assert not m.supported()
        with pytest.raises(RuntimeError, match="node-level head"):
            batching.refuse_node_level(m, "fit_resident")
    assert "node-level" not in (_hscn("graph", vl="GAT").resident_reason() or "")
    assert _mpnn("graph").resident_reason() is None
    m = _hscn()
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="node-level head"):
        m({"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, {}, None)        # before any launch
    m.engine = "auto"
    assert m._resident_plan({"local": torch.zeros(3, 9)}, {}, None) is None
    v = _hscn(vl="GAT")
    v.engine = "resident"
    with pytest.raises(RuntimeError, match="node-level head"):
        v({"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, {}, None)
    p = _mpnn()
    p.engine = "resident"
    with pytest.raises(RuntimeError, match="node-level head"):
        p(None)


def test_resident_steps_fit_resident_and_the_evaluator_refuse_before_anything_runs():
    from types import SimpleNamespace
    from graph_hscn.step import MPNNResidentTrainStep, ResidentTrainStep, VLResidentTrainStep
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    batch = SimpleNamespace(x_dict={"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, edge_index_dict={},
                            x=torch.zeros(3, 9))
    with pytest.raises(RuntimeError, match="node-level head"):
        ResidentTrainStep(_hscn(), batch, "cross_entropy")
    with pytest.raises(RuntimeError, match="node-level head"):
        VLResidentTrainStep(_hscn(vl="GAT"), batch, "cross_entropy")
    with pytest.raises(RuntimeError, match="node-level head"):
        MPNNResidentTrainStep(_mpnn(), batch, "cross_entropy")
    cfg = SimpleNamespace(loss_fn="weighted_cross_entropy", epochs=1, eval_period=1, patience=1, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False)
    for m in (_hscn(), _mpnn()):
        with pytest.raises(RuntimeError, match="node-level head"):
            fit_resident(None, opt, cfg, [None] * 4, None, m, 2)
        with pytest.raises(RuntimeError, match="node-level head"):
            DeviceEvaluator([None] * 4, m, "weighted_cross_entropy", 2)


def test_bad_arguments_are_refused_without_a_gpu():
    from graph_hscn import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(512)
    p = ctypes.addressof(buf)
    BAD, UNSUPPORTED, WORKSPACE = -1, -3, -2
    cw = L.hscn_class_weights
    assert cw(None, 4, 3, -100, 0, None, p, p, p, p, None) == BAD
    assert cw(p, 0, 3, -100, 0, None, p, p, p, p, None) == BAD
    assert cw(p, 1 << 31, 3, -100, 0, None, p, p, p, p, None) == BAD
    assert cw(p, 4, 0, -100, 0, None, p, p, p, p, None) == BAD
    assert cw(p, 4, 1025, -100, 0, None, p, p, p, p, None) == BAD
    assert cw(p, 4, 3, -100, 3, None, p, p, p, p, None) == BAD                       # an unknown mode
    assert cw(p, 4, 3, -100, 1, None, p, p, p, p, None) == BAD                       # given weights, none given
    for k in (6, 7, 8, 9):                                                           # counts, weight, denom, flags
        args = [p, 4, 3, -100, 0, None, p, p, p, p, None]
        args[k] = None
        assert cw(*args) == BAD
    ex = L.hscn_softmax_nll_fwd_ex
    good = [p, p, 4, 3, None, -100, p, p, None, p, p, None, 0, None]
    for k in (0, 1, 6, 7, 9, 10):                                                    # pred, target, denom, loss, grad, flags
        args = list(good)
        args[k] = None
        assert ex(*args) == BAD
    for k, v in ((2, 0), (3, 0), (3, 1025), (2, (1 << 40) + 1)):
        args = list(good)
        args[k] = v
        assert ex(*args) == BAD
    args = list(good)
    args[2] = 257                                                                    # a fold without a workspace
    assert ex(*args) == BAD
    args[11], args[12] = p, 4
    assert ex(*args) == WORKSPACE
    fwd = L.hscn_node_head_fwd
    assert fwd(p, p, p, p, p, 0, 16, 4, 0, p, None) == 0                             # N = 0: nothing to do
    assert fwd(p, p, p, p, p, -1, 16, 4, 0, p, None) == BAD
    assert fwd(None, p, p, p, p, 4, 16, 4, 0, p, None) == BAD
    assert fwd(p, None, p, p, p, 4, 16, 4, 0, p, None) == BAD
    assert fwd(p, p, p, p, p, 4, 16, 4, 0, None, None) == BAD
    assert fwd(p, p, p, p, p, 4, 16, 4, 4, p, None) == BAD                           # an unknown activation
    assert fwd(p, p, p, p, p, 4, 8, 4, 0, p, None) == UNSUPPORTED
    assert fwd(p, p, p, p, p, 4, 16, 65, 0, p, None) == UNSUPPORTED
    bwd = L.hscn_node_head_bwd
    good = [p, p, p, p, p, p, None, 4, 16, 4, 0, None, p, p, p, p, 0, p, 1 << 20, None]
    for k in (0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 17):
        args = list(good)
        args[k] = None
        assert bwd(*args) == BAD
    for k, v in ((7, 0), (7, (1 << 31) + 1), (10, -1), (10, 4), (16, 2)):
        args = list(good)
        args[k] = v
        assert bwd(*args) == BAD
    for k, v in ((8, 128), (9, 0), (9, 65)):
        args = list(good)
        args[k] = v
        assert bwd(*args) == UNSUPPORTED
    args = list(good)
    args[18] = 20 * 17 * 4 - 1
    assert bwd(*args) == WORKSPACE
