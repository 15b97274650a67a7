"""Link-level tasks, host side: config fields and models, the link-labelled synthetic shape, collation of candidate
pairs, ``check_link_labels``, the CPU restatement of the ranking metric worked by hand, the envelope exports and the
refusals of the resident engines.  CPU only: nothing here launches."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _hscn(task_level="link", vl=None, H=16, C=16):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, H, C, 3, vl_conv=vl, task_level=task_level)


def _mpnn(task_level="link"):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    return MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 16, 3, task_level=task_level)


def test_configs_and_models_accept_link_and_still_refuse_edge():
    from graph_hscn.config.config import HSCNConfig, MPNNConfig, TrainingConfig
    from graph_hscn.model.hscn import build_hscn
    from graph_hscn.model.mpnn import build_mpnn
    m = build_hscn(HSCNConfig("relu", task_level="link"), 9, 16)
    assert m.task_level == "link" and m.node_head is not None
    assert build_mpnn(MPNNConfig("gcn", "relu", task_level="link"), 9, 16).task_level == "link"
    assert sorted(m.state_dict()) == sorted(build_hscn(HSCNConfig("relu"), 9, 16).state_dict())
    assert sorted(_mpnn().state_dict()) == sorted(_mpnn("graph").state_dict())
    for bad in (lambda: HSCNConfig("relu", task_level="edge"), lambda: MPNNConfig("gcn", "relu", task_level="edge"),
                lambda: _hscn("edge"), lambda: _mpnn("edge")):
        with pytest.raises(ValueError):
            bad()
    for metric in ("mrr", "hits@1", "hits@3", "hits@10"):
        assert TrainingConfig("hscn", "cross_entropy", metric).metric == metric
    with pytest.raises(RuntimeError, match="link-level"):
        _hscn("node").embed({}, {}, None)


def _hops(n, ei):
    adj = np.zeros((n, n), dtype=bool)
    adj[ei[0], ei[1]] = True
    dist = np.full((n, n), n)
    np.fill_diagonal(dist, 0)
    reach = np.eye(n, dtype=bool)
    for d in range(1, n):
        new = (reach.astype(np.int64) @ adj.astype(np.int64) > 0) & (dist == n)
        dist[new] = d
        reach = reach | new
    return dist


def test_link_labelled_shape_is_seeded_and_keeps_the_graphs_of_pcqm_contact():
    from graph_hscn.data import check_link_labels
    from graph_hscn.loader.synthetic import LINK_SHAPES, NODE_SHAPES, SHAPES, make_dataset
    assert "pcqm_contact_link" in LINK_SHAPES and "pcqm_contact_link" not in SHAPES
    assert "pcqm_contact_link" not in NODE_SHAPES and SHAPES["pcqm_contact"].task == "regression"
    a, b = make_dataset("pcqm_contact_link", 64, seed=0), make_dataset("pcqm_contact_link", 64, seed=0)
    plain = make_dataset("pcqm_contact", 64, seed=0)
    shares, empty = [], 0
    for g, h, p in zip(a, b, plain):
        assert torch.equal(g.edge_label_index, h.edge_label_index) and torch.equal(g.edge_label, h.edge_label)
        assert torch.equal(g.x, p.x) and torch.equal(g.edge_index, p.edge_index) and g.num_nodes == p.num_nodes
        assert p.y.shape == (1, 1) and g.y is None                                     # the graph-level shape is as it was
        check_link_labels(g)
        n, idx, lab = g.num_nodes, g.edge_label_index, g.edge_label
        assert idx.dtype == torch.int64 and lab.dtype == torch.float32 and lab.shape == (idx.size(1),)
        dist = _hops(n, g.edge_index.numpy())
        assert int(torch.unique(idx[0] * n + idx[1]).numel()) == idx.size(1)           # distinct
        assert bool((torch.from_numpy(dist)[idx[0], idx[1]] >= 2).all())
        assert idx.size(1) == int((dist >= 2).sum())                                   # every such ordered pair
        dense = torch.full((n, n), -1.0)
        dense[idx[0], idx[1]] = lab
        assert torch.equal(dense, dense.T)                                             # symmetric labels
        empty += int(lab.sum() == 0)
        shares.append(float(lab.mean()))
    assert empty >= 1
    assert 0.02 <= float(np.mean(shares)) <= 0.20
    other = make_dataset("pcqm_contact_link", 2, seed=1)
    assert not torch.equal(other[0].x, a[0].x)


def _link_graph(n, pairs, labels, F=3, seed=0):
    from graph_hscn.data import Data
    g = torch.Generator().manual_seed(seed)
    return Data(x=torch.randn(n, F, generator=g), edge_index=torch.zeros(2, 0, dtype=torch.int64), num_nodes=n,
                edge_label_index=torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2).T.contiguous(),
                edge_label=torch.tensor(labels, dtype=torch.float32))


def test_batch_collation_offsets_pair_ptr_and_round_trip():
    from graph_hscn.data import Batch
    gs = [_link_graph(3, [(0, 2), (2, 0)], [1, 0]), _link_graph(1, [], []), _link_graph(4, [(3, 0), (1, 3), (0, 1)], [0, 1, 1])]
    b = Batch.from_data_list(gs)
    assert b.edge_label_index.tolist() == [[0, 2, 7, 5, 4], [2, 0, 4, 7, 5]]
    assert b.edge_label.tolist() == [1, 0, 0, 1, 1]
    assert b.pair_ptr32.dtype == torch.int32 and b.pair_ptr32.tolist() == [0, 2, 2, 5] and b.max_pairs == 3
    for g, back in zip(gs, b.to_data_list()):
        assert torch.equal(back.edge_label_index, g.edge_label_index) and torch.equal(back.edge_label, g.edge_label)
        assert back.edge_label_index.dtype == torch.int64 and back.edge_label_index.shape[0] == 2
        assert torch.equal(back.x, g.x)
    plain = Batch.from_data_list([_link_graph(3, [], []).__class__(x=torch.zeros(2, 1), edge_index=torch.zeros(2, 0, dtype=torch.int64))])
    assert "edge_label_index" not in plain and "pair_ptr32" not in plain
    from graph_hscn.data import Data
    with pytest.raises(ValueError, match="some graphs"):
        Batch.from_data_list([gs[0], Data(x=torch.zeros(2, 3), edge_index=torch.zeros(2, 0, dtype=torch.int64))])


def test_two_node_graphs_do_not_turn_the_pair_index_into_a_per_node_extra():
    from graph_hscn.data import Batch
    gs = [_link_graph(2, [(0, 1), (1, 0)], [1, 1], seed=s) for s in range(3)]      # edge_label_index is [2, 2]: n rows
    b = Batch.from_data_list(gs)
    assert b.edge_label_index.shape == (2, 6)
    assert b.edge_label_index.tolist() == [[0, 1, 2, 3, 4, 5], [1, 0, 3, 2, 5, 4]]
    assert b.edge_label.shape == (6,) and b.pair_ptr32.tolist() == [0, 2, 4, 6]
    for g, back in zip(gs, b.to_data_list()):
        assert torch.equal(back.edge_label_index, g.edge_label_index) and torch.equal(back.edge_label, g.edge_label)


def test_hetero_collation_and_loaders_carry_the_pairs_on_the_local_type():
    from graph_hscn.config.config import DataConfig, HSCNConfig
    from graph_hscn.data import Batch, HeteroBatch
    from graph_hscn.loader.hetero_data import generate_hetero_data, hetero_from_clusters, hetero_loaders
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("pcqm_contact_link", 6, seed=1)
    rng = np.random.default_rng(0)
    clusters = [rng.integers(0, 4, g.num_nodes) for g in graphs]
    split = {"train": torch.tensor([0, 1, 2, 3]), "val": torch.tensor([4]), "test": torch.tensor([5])}
    cfg = DataConfig("pcqm_contact", batch_size=2, num_workers=0, task_level="link")
    assert cfg.task_level == "link"
    hs = generate_hetero_data(clusters, graphs, split, cfg, HSCNConfig("relu", num_clusters=4))
    for g, h in zip(graphs, hs):
        assert torch.equal(h["local"].edge_label_index, g.edge_label_index)
        assert torch.equal(h["local"].edge_label, g.edge_label)
    assert "edge_label_index" not in hetero_from_clusters(graphs[0], clusters[0], 4)["local"]     # graph level: not copied
    hb, b = HeteroBatch.from_data_list(hs[:3]), Batch.from_data_list(graphs[:3])
    for k in ("edge_label_index", "edge_label", "pair_ptr32"):
        assert torch.equal(getattr(hb["local"], k), getattr(b, k))
    assert hb["local"].max_pairs == b.max_pairs
    assert "edge_label_index" not in hb["virtual"]
    batch = next(iter(hetero_loaders(cfg, hs, split)[1]))
    assert torch.equal(batch["local"].edge_label, graphs[4].edge_label)
    cfg.task_level = "edge"
    with pytest.raises(NotImplementedError):
        generate_hetero_data(clusters, graphs, split, cfg, HSCNConfig("relu", num_clusters=4))
    with pytest.raises(NotImplementedError):
        hetero_loaders(cfg, hs, split)


def test_check_link_labels_rejects_malformed_graphs():
    from graph_hscn.data import Data, check_link_labels
    check_link_labels(_link_graph(3, [(0, 2), (2, 0), (1, 1)], [1, 0, 1]))
    check_link_labels(_link_graph(3, [], []))
    with pytest.raises(ValueError, match="twice"):
        check_link_labels(_link_graph(3, [(0, 2), (1, 0), (0, 2)], [1, 0, 1]))
    with pytest.raises(ValueError, match="outside"):
        check_link_labels(_link_graph(3, [(0, 3)], [1]))
    with pytest.raises(ValueError, match="outside"):
        check_link_labels(_link_graph(3, [(-1, 2)], [1]))
    with pytest.raises(ValueError, match="0 or 1"):
        check_link_labels(_link_graph(3, [(0, 2)], [0.5]))
    g = _link_graph(3, [(0, 2)], [1])
    g.edge_label_index = g.edge_label_index.to(torch.int32)
    with pytest.raises(ValueError, match="int64"):
        check_link_labels(g)
    g = _link_graph(3, [(0, 2)], [1])
    g.edge_label = g.edge_label.double()
    with pytest.raises(ValueError, match="float32"):
        check_link_labels(g)
    g = _link_graph(3, [(0, 2)], [1])
    g.edge_label_index = g.edge_label_index.T.contiguous()
    with pytest.raises(ValueError, match=r"\[2, P\]"):
        check_link_labels(g)
    g = _link_graph(3, [(0, 2), (1, 2)], [1, 1])
    g.edge_label = g.edge_label[:1]
    with pytest.raises(ValueError, match="one label per"):
        check_link_labels(g)
    with pytest.raises(ValueError, match="carries"):
        check_link_labels(Data(x=torch.zeros(2, 1), edge_index=torch.zeros(2, 0, dtype=torch.int64)))


def test_device_datasets_refuse_link_labelled_graphs_by_name():
    from graph_hscn.loader.device_dataset import DeviceGraphDataset, DeviceHeteroDataset
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    g = _link_graph(3, [(0, 2)], [1])
    with pytest.raises(ValueError, match="edge_label_index"):
        DeviceGraphDataset([g], "cpu", 1)
    with pytest.raises(ValueError, match="edge_label_index"):
        DeviceHeteroDataset([hetero_from_clusters(g, [0, 1, 0], 2, "link")], "cpu", 1)


# ---- link_rank_counts by hand ---------------------------------------------------------------------------------------
# One 4-node graph, z = [[2, 0], [1, 0], [1, 0], [0, 1]]: the scores s(a, b) = <z_a, z_b> are
#        0  1  2  3
#   0  [ 4  2  2  0 ]
#   1  [ 2  1  1  0 ]
#   2  [ 2  1  1  0 ]
#   3  [ 0  0  0  1 ]
# candidates (u, v): (0,1)+ (0,2)+ (0,3)- (1,2)+ (3,0)+ (1,3)-
_Z = torch.tensor([[2.0, 0.0], [1.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (3, 0), (1, 3)]
_LABELS = [1, 1, 0, 1, 1, 0]


def _by_hand(filter):
    from graph_hscn.metrics import link_rank_counts
    idx = torch.tensor(_PAIRS).T.contiguous()
    return link_rank_counts(_Z, torch.tensor([0, 4]), torch.tensor([0, 6]), idx, torch.tensor(_LABELS, dtype=torch.float32),
                            filter)


def test_link_rank_counts_by_hand_for_the_three_filters():
    # filter 0.  (0,1): s = 2 against w in {0, 2, 3} = {4, 2, 0}: g = 1 (the self score), e = 1 (the positive (0,2))
    #            (0,2): the same by symmetry.  (1,2): s = 1 against w in {0, 1, 3} = {2, 1, 0}: g = 1, e = 1 (self).
    #            (3,0): s = 0 against w in {1, 2, 3} = {0, 0, 1}: g = 1 (self), e = 2.
    r2, pg = _by_hand(0)
    assert r2.dtype == torch.int32 and r2.tolist() == [3, 3, -1, 3, 4, -1]
    rr = 2 / 5 + 2 / 5 + 2 / 5 + 2 / 6
    assert pg.dtype == torch.float64 and pg.shape == (1, 5)
    assert pg[0].tolist() == [((2 / 5 + 2 / 5) + 2 / 5) + 2 / 6, 0.0, 4.0, 4.0, 4.0] and abs(float(pg[0, 0]) - rr) < 1e-15
    # filter 1: (0,1) loses its only equal competitor, the positive (0,2): rank2 3 -> 2, that is rank 2.5 -> 2 (the
    # self score still outranks it); (1,2) and (3,0) have no other positive partner
    r2, pg = _by_hand(1)
    assert r2.tolist() == [2, 2, -1, 3, 4, -1]
    assert pg[0].tolist() == [((2 / 4 + 2 / 4) + 2 / 5) + 2 / 6, 0.0, 4.0, 4.0, 4.0]
    # filter 2: the self score goes too.  (0,1): nothing above, nothing equal: rank 1.  (1,2): only w = 0 (score 2) is
    # above: g = 1.  (3,0): w in {1, 2}, both equal: e = 2, rank 2.
    r2, pg = _by_hand(2)
    assert r2.tolist() == [0, 0, -1, 2, 2, -1]
    assert pg[0].tolist() == [((1.0 + 1.0) + 2 / 4) + 2 / 4, 2.0, 4.0, 4.0, 4.0]


def test_a_tie_with_one_negative_is_rank_one_and_a_half():
    from graph_hscn.metrics import link_rank_counts
    z = torch.tensor([[1.0, 0.0], [1.0, 1.0], [1.0, -1.0]])           # s(0, 1) = s(0, 2) = 1; s(0, 0) = 1 as well
    idx = torch.tensor([[0], [1]])
    for filter, want in ((0, 2), (1, 2), (2, 1)):                     # e = 2 with the self score, e = 1 without
        r2, pg = link_rank_counts(z, torch.tensor([0, 3]), torch.tensor([0, 1]), idx, torch.ones(1), filter)
        assert r2.tolist() == [want]
    assert 1 + 0 + 1 / 2 == 1.5 and float(pg[0, 0]) == 2.0 / 3.0       # rank 1.5: reciprocal 2 / (1 + 2)
    assert pg[0].tolist()[1:] == [0.0, 1.0, 1.0, 1.0]                  # rank 1.5 is no hit at 1


def test_a_positive_whose_only_competitor_is_another_positive():
    from graph_hscn.metrics import link_rank_counts
    # 3 nodes, z_0 = (0.5, 0): s(0, .) = [0.25, 0.5, 1].  Positives (0,1) and (0,2).  For (0,1) the self score is below
    # and the only node above is w = 2, itself a positive partner of 0.
    z = torch.tensor([[0.5, 0.0], [1.0, 5.0], [2.0, 7.0]])
    idx = torch.tensor([[0, 0], [1, 2]])
    args = (z, torch.tensor([0, 3]), torch.tensor([0, 2]), idx, torch.ones(2))
    r2, _ = link_rank_counts(*args, 0)
    assert r2.tolist() == [2, 0]                                       # (0,1): rank 2 unfiltered
    r2, _ = link_rank_counts(*args, 1)
    assert r2.tolist() == [0, 0]                                       # rank 1 filtered
    r2, _ = link_rank_counts(*args, 2)
    assert r2.tolist() == [0, 0]


def test_the_self_score_outranks_the_positive_under_filters_0_and_1_only():
    from graph_hscn.metrics import link_rank_counts
    z = torch.tensor([[3.0, 0.0], [1.0, 0.0], [0.0, 1.0]])            # s(0, .) = [9, 3, 0]
    idx = torch.tensor([[0], [1]])
    got = [link_rank_counts(z, torch.tensor([0, 3]), torch.tensor([0, 1]), idx, torch.ones(1), f)[0].tolist() for f in (0, 1, 2)]
    assert got == [[2], [2], [0]]


def test_graph_and_pooled_averaging_on_a_two_graph_example_and_graphs_without_positives():
    from graph_hscn.metrics import eval_link_ranks, link_means, link_rank_counts
    # graph A: the 4-node graph above, filter 2: reciprocal ranks 1, 1, 1/2, 1/2 (4 positives), hits@1 = 2 of 4
    # graph B: 2 nodes, no positives (one negative candidate)
    # graph C: 3 nodes, z = [(1, 0), (1, 0), (3, 0)], one positive (0, 1): s = 1, w = 2 scores 3: rank 2, reciprocal 1/2
    z = torch.cat([_Z, torch.tensor([[1.0, 1.0], [1.0, 2.0]]), torch.tensor([[1.0, 0.0], [1.0, 0.0], [3.0, 0.0]])])
    idx = torch.tensor(_PAIRS + [(4, 5)] + [(6, 7)]).T.contiguous()
    lab = torch.tensor(_LABELS + [0] + [1], dtype=torch.float32)
    ptr, pptr = torch.tensor([0, 4, 6, 9]), torch.tensor([0, 6, 7, 8])
    r2, pg = link_rank_counts(z, ptr, pptr, idx, lab, 2)
    assert r2.tolist() == [0, 0, -1, 2, 2, -1, -1, 2]
    assert pg.tolist() == [[3.0, 2.0, 4.0, 4.0, 4.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 1.0, 1.0, 1.0]]
    graph = link_means(pg, "graph")
    pooled = link_means(pg, "pooled")
    assert graph == ((3.0 / 4 + 0.5 / 1) / 2, (2.0 / 4 + 0.0) / 2, 1.0, 1.0)          # B is left out: two graphs
    assert pooled == (3.5 / 5, 2.0 / 5, 1.0, 1.0)                                     # B adds nothing: five positives
    assert graph[0] == 0.625 and pooled[0] == 0.7 and graph[1] == 0.25 and pooled[1] == 0.4
    assert eval_link_ranks(z, ptr, pptr, idx, lab, 2, "graph") == graph
    with pytest.raises(RuntimeError, match="No positive pair"):
        link_means(pg[1:2], "graph")
    with pytest.raises(ValueError):
        link_means(pg, "macro")
    with pytest.raises(ValueError):
        link_rank_counts(z, ptr, pptr, idx, lab, 3)
    with pytest.raises(ValueError, match="0 or 1"):
        link_rank_counts(z, ptr, pptr, idx, lab * 0.5, 0)
    bad = idx.clone()
    bad[1, 0] = 5                                                                      # a pair that leaves graph A
    with pytest.raises(IndexError):
        link_rank_counts(z, ptr, pptr, bad, lab, 0)


def test_float32_embeddings_stay_float32_and_others_become_float64():
    from graph_hscn.metrics import link_rank_counts
    idx = torch.tensor(_PAIRS).T.contiguous()
    lab = torch.tensor(_LABELS, dtype=torch.float32)
    a = link_rank_counts(_Z, torch.tensor([0, 4]), torch.tensor([0, 6]), idx, lab, 0)
    b = link_rank_counts(_Z.to(torch.int64), torch.tensor([0, 4]), torch.tensor([0, 6]), idx, lab, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- envelopes and refusals ------------------------------------------------------------------------------------------

def test_pair_envelopes_at_their_edges():
    from graph_hscn import _hip
    L = _hip.lib()
    for D, ok in ((0, 0), (4, 1), (6, 0), (8, 1), (12, 1), (16, 1), (60, 1), (64, 1), (68, 0), (128, 0), (-4, 0)):
        assert L.hscn_pair_dot_supported(D) == ok
    for D, per in ((4, 256), (8, 128), (12, 64), (16, 64), (20, 32), (32, 32), (36, 16), (64, 16), (6, 0)):
        assert L.hscn_pair_dot_pairs_per_workgroup(D) == per
    for D, rows in ((4, 3840), (12, 960), (16, 960), (64, 240), (6, 0)):
        assert L.hscn_pair_rank_lds_max_nodes(D) == rows
    assert L.hscn_pair_rank_supported(240, 64) == 1 and L.hscn_pair_rank_supported(241, 64) == 2
    assert L.hscn_pair_rank_supported(0, 4) == 1 and L.hscn_pair_rank_supported(53, 6) == 0
    assert L.hscn_pair_rank_supported(-1, 16) == 0
    assert L.hscn_pair_rank_max_workgroups() == 1024


def test_bad_arguments_are_refused_without_a_gpu():
    from graph_hscn import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 15) & ~15
    BAD, UNSUPPORTED = -1, -3
    fwd = L.hscn_pair_dot_fwd
    assert fwd(p, p, 4, 0, 16, p, p, None) == 0                                      # P = 0: nothing to do
    assert fwd(None, None, 4, 0, 16, None, p, None) == 0
    assert fwd(p, p, 4, 3, 16, p, None, None) == BAD                                 # no flag word
    assert fwd(None, p, 4, 3, 16, p, p, None) == BAD
    assert fwd(p, None, 4, 3, 16, p, p, None) == BAD
    assert fwd(p, p, 4, 3, 16, None, p, None) == BAD
    assert fwd(p, p, -1, 3, 16, p, p, None) == BAD
    assert fwd(p, p, 4, 1 << 31, 16, p, p, None) == BAD
    assert fwd(p + 4, p, 4, 3, 16, p, p, None) == BAD                                # rows move as float4
    assert fwd(p, p, 4, 3, 6, p, p, None) == UNSUPPORTED
    assert fwd(p, p, 4, 3, 68, p, p, None) == UNSUPPORTED
    bwd = L.hscn_pair_dot_bwd
    good = [p, p, p, None, p, p, p, p, 4, 3, 16, p, None]
    for k in (0, 1, 2, 4, 5, 6, 7, 11):
        args = list(good)
        args[k] = None
        assert bwd(*args) == BAD
    for k, v in ((8, 0), (8, 1 << 31), (9, -1), (0, p + 4), (11, p + 8)):
        args = list(good)
        args[k] = v
        assert bwd(*args) == BAD
    args = list(good)
    args[10] = 6
    assert bwd(*args) == UNSUPPORTED
    rank = L.hscn_pair_rank
    good = [p, p, p, p, p, p, p, 2, 4, 3, 16, 1, 0, None, p, p, None]
    assert rank(p, p, p, p, p, p, p, 0, 4, 3, 16, 1, 0, None, p, p, None) == 0       # B = 0: nothing to do
    for k in (0, 1, 2, 3, 4, 5, 6, 14, 15):
        args = list(good)
        args[k] = None
        assert rank(*args) == BAD
    for k, v in ((11, 3), (11, -1), (7, -1), (8, 1 << 31), (0, p + 4)):
        args = list(good)
        args[k] = v
        assert rank(*args) == BAD
    args = list(good)
    args[10] = 68
    assert rank(*args) == UNSUPPORTED
    args = list(good)
    args[5] = args[6] = None                                                         # no positives' CSR: filter 0 only
    assert rank(*args) == BAD
    red = L.hscn_pair_rank_reduce
    assert red(None, 2, 0, None, None, p, p, None) == BAD
    assert red(p, 2, 2, None, None, p, p, None) == BAD                               # an unknown averaging
    assert red(p, 2, 0, p, None, p, p, None) == BAD                                  # half an accumulator
    assert red(p, 2, 0, None, None, None, p, None) == BAD
    assert red(p, 2, 0, None, None, p, None, None) == BAD


def test_link_level_models_name_the_head_and_the_resident_engines_refuse():
    from graph_hscn.train import batching
    for m in (_hscn(), _hscn(vl="GAT"), _mpnn()):
        assert batching.link_level(m) and not batching.node_level(m)
        assert "link-level head" in m.resident_reason()
        assert not m.supported()
        with pytest.raises(RuntimeError, match="link-level head"):
            batching.refuse_link_level(m, "fit_resident")
        batching.refuse_node_level(m, "fit_resident")                                # not its business
    batching.refuse_link_level(_hscn("node"), "fit_resident")
    batching.refuse_link_level(_mpnn("graph"), "fit_resident")
    assert "node-level head" in _hscn("node").resident_reason()                      # word for word as it was
    m = _hscn()
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="link-level head"):
        m({"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, {}, None)      # before any launch
    with pytest.raises(RuntimeError, match="link-level head"):
        batching.forward(m, None)
    m.engine = "auto"
    assert m._resident_plan({"local": torch.zeros(3, 9)}, {}, None) is None
    v = _hscn(vl="GAT")
    v.engine = "resident"
    with pytest.raises(RuntimeError, match="link-level head"):
        v({"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, {}, None)
    p = _mpnn()
    p.engine = "resident"
    with pytest.raises(RuntimeError, match="link-level head"):
        p(None)


def test_resident_steps_fit_resident_the_evaluator_and_the_captured_step_refuse(monkeypatch):
    from graph_hscn import _hip
    from graph_hscn.replay import CapturedStep
    from graph_hscn.step import MPNNResidentTrainStep, ResidentTrainStep, VLResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident

    def no_library():
        raise AssertionError("the refusal must come before the library is touched")

    monkeypatch.setattr(_hip, "lib", no_library)
    batch = SimpleNamespace(x_dict={"local": torch.zeros(3, 9), "virtual": torch.zeros(1, 9)}, edge_index_dict={},
                            x=torch.zeros(3, 9))
    with pytest.raises(RuntimeError, match="link-level head"):
        ResidentTrainStep(_hscn(), batch, "cross_entropy")
    with pytest.raises(RuntimeError, match="link-level head"):
        VLResidentTrainStep(_hscn(vl="GAT"), batch, "cross_entropy")
    with pytest.raises(RuntimeError, match="link-level head"):
        MPNNResidentTrainStep(_mpnn(), batch, "cross_entropy")
    cfg = SimpleNamespace(loss_fn="cross_entropy", epochs=1, eval_period=1, patience=1, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False)
    for m in (_hscn(), _mpnn()):
        with pytest.raises(RuntimeError, match="link-level head"):
            fit_resident(None, opt, cfg, [None] * 4, None, m, 2)
        with pytest.raises(RuntimeError, match="link-level head"):
            DeviceEvaluator([None] * 4, m, "cross_entropy", 2)
        with pytest.raises(RuntimeError, match="link-level head"):
            batching.resident_step(m, batch, "cross_entropy")
        with pytest.raises(RuntimeError, match="link-level head"):
            CapturedStep(m, SimpleNamespace(batch=batch), "cross_entropy")


def test_train_loop_takes_the_ranking_metric_of_a_link_level_model_by_keyword():
    from graph_hscn.config.config import TrainingConfig
    from graph_hscn.train import train as T
    assert T._link_metric_of(TrainingConfig("hscn", "cross_entropy", "hits@3")) == "hits@3"
    assert T._link_metric_of(TrainingConfig("hscn", "cross_entropy", "ap")) == "mrr"
    assert T._link_ranks(_mpnn("graph"), None, None) == (None, None)
    fn = lambda t, s: 0.0
    assert T._link_ranks(_mpnn("graph"), fn, None) == (None, None)                  # metric_fn is what it was
    with pytest.raises(ValueError, match="link-level"):
        T._link_ranks(_mpnn("graph"), None, "mrr")
    acc, name = T._link_ranks(_mpnn(), None, None)
    assert name == "mrr" and acc.filter == 1 and acc.averaging == "graph"
    assert T._link_ranks(_mpnn(), None, "hits@10")[1] == "hits@10"
    with pytest.raises(ValueError, match="scored by"):
        T._link_ranks(_mpnn(), None, "ap")
    with pytest.raises(ValueError, match="link_metric="):
        T._link_ranks(_mpnn(), fn, None)
    assert not hasattr(_mpnn(), "last_embedding") and not hasattr(_hscn(), "last_embedding")


def test_link_rank_counts_ranks_scores_given_from_elsewhere():
    from graph_hscn.metrics import link_rank_counts
    idx = torch.tensor(_PAIRS).T.contiguous()
    lab = torch.tensor(_LABELS, dtype=torch.float32)
    args = (_Z, torch.tensor([0, 4]), torch.tensor([0, 6]), idx, lab, 0)
    same = link_rank_counts(*args, score=lambda zg: zg @ zg.T)
    assert torch.equal(same[0], link_rank_counts(*args)[0])
    flipped = link_rank_counts(*args, score=lambda zg: -(zg @ zg.T))
    # negated scores.  (0,1): -2 against {-4, -2, 0}: g = 1, e = 1.  (1,2): -1 against {-2, -1, 0}: g = 1, e = 1.
    # (3,0): 0 against {0, 0, -1}: e = 2, where the product's scores gave g = 1, e = 2
    assert flipped[0].tolist() == [3, 3, -1, 3, 2, -1]
