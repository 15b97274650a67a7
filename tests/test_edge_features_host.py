"""Edge features without a GPU: the containers and generators carry ``edge_attr``, the float64 restatement of GINEConv
is right on a case worked by hand, the "gine" baseline is wired as stated and refused where it cannot run, and the new
entry points check their arguments before any launch."""
import numpy as np
import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT, MPNNConfig
from graph_hscn.data import Batch, Data
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.mpnn import build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GINE, GINEConv, Linear
from tests import gine_oracle as GO


def _graph(n, e, de, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    ea = torch.randn(e, de, generator=g).to(dtype) if dtype.is_floating_point else torch.randint(0, 5, (e, de), generator=g)
    return Data(x=torch.randn(n, 4, generator=g), edge_index=torch.randint(0, n, (2, e), generator=g),
                y=torch.randn(1, 2, generator=g), edge_attr=ea)


# --------------------------------------------------------------------------- #
# 1. collate round trip
# --------------------------------------------------------------------------- #
def test_collate_round_trip_keeps_every_graphs_edge_attr():
    graphs = [_graph(5, 7, 3, 0), _graph(6, 6, 3, 1),            # E == num_nodes: not a per-node extra
              _graph(4, 0, 3, 2), _graph(3, 9, 3, 3, torch.int64)]
    graphs[3].edge_attr = graphs[3].edge_attr.float()
    b = Batch.from_data_list(graphs)
    assert b.edge_attr.shape == (22, 3)
    assert torch.equal(b.edge_attr, torch.cat([g.edge_attr for g in graphs], 0))
    back = b.to_data_list()
    assert len(back) == 4
    for g, h in zip(graphs, back):
        assert torch.equal(h.edge_attr, g.edge_attr) and h.edge_attr.shape == g.edge_attr.shape
        assert torch.equal(h.edge_index, g.edge_index) and torch.equal(h.x, g.x)
    assert back[2].edge_attr.shape == (0, 3)
    ints = Batch.from_data_list([_graph(3, 4, 3, 4, torch.int64), _graph(3, 2, 3, 5, torch.int64)])
    assert ints.edge_attr.dtype == torch.int64 and ints.edge_attr.shape == (6, 3)
    # a batch without edge features has none
    plain = Batch.from_data_list([Data(x=g.x, edge_index=g.edge_index, y=g.y) for g in graphs])
    assert "edge_attr" not in plain or plain.edge_attr is None
    assert all("edge_attr" not in g or g.edge_attr is None for g in plain.to_data_list())


def test_collate_refuses_mixed_lists_and_malformed_edge_attr():
    a, b = _graph(5, 7, 3, 0), _graph(6, 6, 3, 1)
    with pytest.raises(ValueError, match="some graphs"):
        Batch.from_data_list([a, Data(x=b.x, edge_index=b.edge_index, y=b.y)])
    wrong_rows = Data(x=b.x, edge_index=b.edge_index, y=b.y, edge_attr=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="rows"):
        Batch.from_data_list([a, wrong_rows])
    flat = Data(x=b.x, edge_index=b.edge_index, y=b.y, edge_attr=torch.zeros(6))
    with pytest.raises(ValueError, match=r"\[E, De\]"):
        Batch.from_data_list([a, flat])


def test_to_device_casts_integer_bond_features():
    from graph_hscn.train import batching
    model = build_mpnn(MPNNConfig("gine", "relu"), 9, 10)
    b = batching.to_device(model, Batch.from_data_list(make_dataset("peptides_func", 2, 0, edge_features=True)), "cpu")
    assert b.edge_attr.dtype == torch.float32 and b.x.dtype == torch.float32


# --------------------------------------------------------------------------- #
# 2. generators
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", ["peptides_func", "pascalvoc_sp", "pascalvoc_sp_node", "pcqm_contact_link"])
def test_generators_draw_edge_features_from_a_stream_of_their_own(name):
    plain = make_dataset(name, 6, 3)
    feat = make_dataset(name, 6, 3, edge_features=True)
    atom = name.startswith(("peptides", "pcqm"))
    for p, f in zip(plain, feat):
        assert "edge_attr" not in p or p.edge_attr is None
        assert torch.equal(p.x, f.x) and p.x.dtype == f.x.dtype
        assert torch.equal(p.edge_index, f.edge_index)
        if name.endswith("_link"):
            assert torch.equal(p.edge_label_index, f.edge_label_index) and torch.equal(p.edge_label, f.edge_label)
        else:
            assert torch.equal(p.y, f.y) and p.y.dtype == f.y.dtype
        ea, E = f.edge_attr, f.edge_index.size(1)
        assert ea.shape == ((E, 3) if atom else (E, 2))
        assert ea.dtype == (torch.int64 if atom else torch.float32)
        assert torch.equal(f.edge_index[:, 0::2], f.edge_index[:, 1::2].flip(0))     # (i, j), (j, i) are adjacent
        assert torch.equal(ea[0::2], ea[1::2])                                       # ... and share their row
        if atom:
            assert int(ea.min()) >= 0 and all(int(ea[:, c].max()) < card for c, card in enumerate((5, 6, 2)))
    if atom:        # every value of every column occurs somewhere in the six graphs
        allea = torch.cat([f.edge_attr for f in feat])
        assert [int(allea[:, c].max()) + 1 for c in range(3)] == [5, 6, 2]
    # the same seed gives the same features; another seed gives others
    again = make_dataset(name, 6, 3, edge_features=True)
    assert all(torch.equal(a.edge_attr, f.edge_attr) for a, f in zip(again, feat))
    other = make_dataset(name, 6, 4, edge_features=True)
    assert not all(a.edge_attr.shape == f.edge_attr.shape and torch.equal(a.edge_attr, f.edge_attr)
                   for a, f in zip(other, feat))


# --------------------------------------------------------------------------- #
# 3. the restatement on a case worked by hand
# --------------------------------------------------------------------------- #
def test_restatement_known_answer():
    """Three nodes, F = 2, De = 1, eps = 0.5; edges (src -> dst): k0 = 0 -> 1, k1 = 0 -> 1 again, k2 = 2 -> 2 (a loop).

        x = [[1, 3], [3, -4], [1, 0]]     e = [[1], [2], [-1]]     lin.weight = [[1], [-2]]     lin.bias = [0.5, 0]

        t_0 = [0.5 + 1, -2] = [1.5, -2]      pre_0 = x_0 + t_0 = [2.5,  1]     m_0 = [2.5, 1]
        t_1 = [0.5 + 2, -4] = [2.5, -4]      pre_1 = x_0 + t_1 = [3.5, -1]     m_1 = [3.5, 0]     (one negative input)
        t_2 = [0.5 - 1,  2] = [-0.5, 2]      pre_2 = x_2 + t_2 = [0.5,  2]     m_2 = [0.5, 2]

        z_0 = 1.5 [1, 3]                      = [1.5, 4.5]          (no edge arrives)
        z_1 = 1.5 [3, -4] + m_0 + m_1         = [4.5 + 6, -6 + 1]   = [10.5, -5]
        z_2 = 1.5 [1, 0] + m_2                = [2, 2]

    Every number is a dyadic rational: float64 reproduces it exactly.  Without edge k1: z_1 = [7, -5]."""
    d = torch.float64
    x = torch.tensor([[1., 3.], [3., -4.], [1., 0.]], dtype=d)
    ei = torch.tensor([[0, 0, 2], [1, 1, 2]])
    e = torch.tensor([[1.], [2.], [-1.]], dtype=d)
    W = torch.tensor([[1.], [-2.]], dtype=d)
    b = torch.tensor([0.5, 0.], dtype=d)
    pre = GO.pre_activations(x, ei, e, W, b)
    assert torch.equal(pre, torch.tensor([[2.5, 1.], [3.5, -1.], [0.5, 2.]], dtype=d))
    z = GO.aggregate(x, ei, e, W, b, eps=0.5)
    assert torch.equal(z, torch.tensor([[1.5, 4.5], [10.5, -5.], [2., 2.]], dtype=d))
    assert torch.equal(GO.aggregate(x, ei, e, W, b, eps=0.5, skip=1),
                       torch.tensor([[1.5, 4.5], [7., -5.], [2., 2.]], dtype=d))
    # the module form, nn = identity
    m = GO.GINEConvRef(torch.nn.Identity(), 1, 2, eps=0.5).double()
    with torch.no_grad():
        m.lin.weight.copy_(W)
        m.lin.bias.copy_(b)
    assert torch.equal(m(x, ei, e), z)
    mag, n = GO.aggregate_magnitude(x, ei, e, W, b, eps=0.5)
    assert torch.equal(n.flatten(), torch.tensor([5., 7., 6.], dtype=d))                # deg + De + 4
    assert torch.equal(mag[1], torch.tensor([4.5 + 2.5 + 3.5, 6. + 5. + 7.], dtype=d))


# --------------------------------------------------------------------------- #
# 4. model wiring
# --------------------------------------------------------------------------- #
def test_gine_baseline_is_built_as_stated():
    assert CONV_DICT["gine"] is GINE and "gin" not in CONV_DICT
    model = build_mpnn(MPNNConfig("gine", "relu"), 9, 10)
    assert len(model.conv_layers) == 3 and all(type(c) is GINE for c in model.conv_layers)
    assert GINE.uses_edge_attr is True
    widths = [(c.nn[0].in_channels, c.nn[0].out_channels, c.nn[2].in_channels, c.nn[2].out_channels)
              for c in model.conv_layers]
    assert widths == [(9, 16, 16, 16), (16, 16, 16, 16), (16, 10, 10, 10)]
    assert [c.lin.out_channels for c in model.conv_layers] == [9, 16, 16]
    assert all(isinstance(c.lin, Linear) and isinstance(c.nn[0], Linear) for c in model.conv_layers)
    keys = set(model.state_dict().keys())
    assert keys == {f"conv_layers.{i}.{k}" for i in range(3)
                    for k in ("nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "lin.weight", "lin.bias", "eps")}
    assert "eps" in dict(model.conv_layers[0].named_buffers()) and not any(
        n.endswith("eps") for n, _ in model.named_parameters())
    assert float(model.conv_layers[0].eps) == 0.0
    # edge_dim=-1 materialises on first use; an explicit one is sized at once
    assert isinstance(model.conv_layers[0].lin.weight, torch.nn.parameter.UninitializedParameter)
    assert GINE(9, 16, edge_dim=3).lin.weight.shape == (9, 3)
    conv = GINEConv(torch.nn.Sequential(Linear(5, 7)), eps=0.25, edge_dim=2)
    assert conv.lin.weight.shape == (5, 2) and float(conv.eps) == 0.25 and conv.initial_eps == 0.25
    conv.load_state_dict({**conv.state_dict(), "eps": torch.tensor([0.5])})
    assert conv.initial_eps == 0.5


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="train_eps"):
        GINEConv(torch.nn.Sequential(Linear(5, 7)), train_eps=True, edge_dim=2)
    with pytest.raises(NotImplementedError, match="edge_dim"):
        GINEConv(torch.nn.Sequential(Linear(5, 7)))
    model = build_mpnn(MPNNConfig("gine", "relu"), 9, 10)
    reason = model.resident_reason()
    assert reason is not None and "GINE" in reason
    assert not model.supported()
    from graph_hscn.train import batching
    plain = batching.to_device(model, Batch.from_data_list(make_dataset("peptides_func", 2, 0)), "cpu")
    with pytest.raises(ValueError, match="carries no edge_attr"):
        model(plain)
    ints = Batch.from_data_list(make_dataset("peptides_func", 2, 0, edge_features=True))
    ints.x = ints.x.float()
    with pytest.raises(TypeError, match="float32"):
        model(ints)
    # the hetero graph carries no edge features: HSCN refuses the name, not a keyword
    from graph_hscn.model.hscn import HSCN, build_conv_relation
    with pytest.raises(ValueError, match="no edge features"):
        build_conv_relation("GINE", 16)
    with pytest.raises(ValueError, match="no edge features"):
        HSCN("GAT", "GINE", "GCN", ACT_DICT["relu"], 9, 16, 10, 3)
    with pytest.raises(KeyError):
        build_mpnn(MPNNConfig("gin", "relu"), 9, 10)


# --------------------------------------------------------------------------- #
# 5. entry points, without a launch
# --------------------------------------------------------------------------- #
def test_entry_points_check_their_arguments_before_any_launch():
    import ctypes
    from graph_hscn import _hip
    lib = _hip.lib()
    assert [lib.hscn_gine_supported(*a) for a in ((1, 1), (512, 64), (513, 3), (16, 65), (0, 3))] == [1, 1, 0, 0, 0]
    assert lib.hscn_gine_long_row() == Fh.GINE_LONG_ROW and lib.hscn_gine_chunk() == Fh.GINE_CHUNK
    assert (Fh.GINE_MAX_WIDTH, Fh.GINE_MAX_EDGE_DIM) == (512, 64)
    buf = ctypes.create_string_buffer(64)
    here = ctypes.addressof(buf)            # a host buffer standing in for a pointer the checks only compare with NULL
    BADARG, UNSUPPORTED = -1, -3

    def fwd(N, E, F, De, p=here, edge=here):
        return lib.hscn_gine_aggregate_fwd(p, edge, edge, p, edge, p, p, 0.0, p, N, E, F, De, p, None)

    def bwd_x(N, E, F, De, p=here, edge=here):
        return lib.hscn_gine_aggregate_bwd_x(p, edge, edge, p, edge, p, p, 0.0, p, p, N, E, F, De, p, None)

    def bwd_msg(N, E, F, De, p=here):
        return lib.hscn_gine_aggregate_bwd_msg(p, p, p, p, p, p, p, N, E, F, De, p, None)

    for f in (fwd, bwd_x, bwd_msg):
        assert f(-1, 4, 16, 3) == BADARG and f(4, -1, 16, 3) == BADARG
        assert f(4, 4, 0, 3) == BADARG and f(4, 4, 16, 0) == BADARG
        assert f(4, 4, 513, 3) == UNSUPPORTED and f(4, 4, 16, 65) == UNSUPPORTED
        assert f(4, 4, 16, 3, p=None) == BADARG                       # NULL pointers with E > 0
    assert fwd(4, 4, 16, 3, edge=None) == BADARG and bwd_x(4, 4, 16, 3, edge=None) == BADARG
    assert fwd(0, 0, 16, 3, p=None, edge=None) == 0                   # nothing to do
    assert bwd_x(0, 0, 16, 3, p=None, edge=None) == 0
    assert bwd_msg(4, 0, 16, 3, p=None) == 0
