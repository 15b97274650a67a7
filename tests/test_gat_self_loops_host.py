"""Host-side surface of GATConv(in, out) with PyG's default ``add_self_loops=True`` -- the convolution
``CONV_DICT["gat"]`` gives the MPNN baseline (reference model/mpnn.py:29-32, config/config.py:19-23) -- and the
oracle identity the GPU tests of this operator rest on.  No GPU needed."""
import ctypes

import pytest
import torch


def _dense_gat64(x, W, att_s, att_d, bias, edge_index, slope=0.2):
    """GATConv(heads=1, add_self_loops=True) of ONE graph in float64 with one dense softmax matrix: M[i, j] = number of
    input edges j -> i with j != i (repeated edges count with their multiplicity, input loops do not count), plus the
    identity (the one appended loop per node)."""
    n = x.shape[0]
    h = x.double() @ W.double().t()
    a_s, a_d = h @ att_s.double().view(-1), h @ att_d.double().view(-1)
    M = torch.zeros(n, n, dtype=torch.float64)
    for s, d in edge_index.t().tolist():
        if s != d:
            M[d, s] += 1.0
    M += torch.eye(n, dtype=torch.float64)
    z = a_d.view(-1, 1) + a_s.view(1, -1)
    z = torch.where(z > 0, z, z * slope)
    zmax = torch.where(M > 0, z, torch.full_like(z, -float("inf"))).max(1, keepdim=True).values
    ex = M * torch.exp(z - zmax)
    alpha = ex / (ex.sum(1, keepdim=True) + 1e-16)
    return alpha @ h + bias.double()


def test_build_mpnn_with_gat_constructs():
    """Fails on a tree whose GATConv refuses add_self_loops=True: MPNN calls conv(num_features, hidden)."""
    from graph_hscn.config.config import MPNNConfig
    from graph_hscn.model.mpnn import build_mpnn
    from graph_hscn.nn.conv import GATConv
    m = build_mpnn(MPNNConfig(conv_type="gat", activation="relu"), 9, 10)
    assert len(m.conv_layers) == m.num_layers
    assert all(isinstance(c, GATConv) and c.add_self_loops for c in m.conv_layers)
    assert m.conv_layers[0].lin_src.weight.shape[1] == 9 and m.conv_layers[-1].out_channels == 10


def test_state_dict_shared_weight_and_parameter_count():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.nn.conv import GATConv
    c = GATConv(9, 16)
    assert c.lin_dst is c.lin_src
    assert sorted(c.state_dict()) == ["att_dst", "att_src", "bias", "lin_dst.weight", "lin_src.weight"]
    assert c.state_dict()["lin_dst.weight"].data_ptr() == c.state_dict()["lin_src.weight"].data_ptr()
    assert sum(1 for _ in c.parameters()) == 4
    assert sum(p.numel() for p in c.parameters()) == 9 * 16 + 3 * 16
    F, H, C, L = 9, 16, 10, 3
    m = MPNN(CONV_DICT["gat"], ACT_DICT["relu"], F, H, C, L)
    dims = [(F, H)] + [(H, H)] * (L - 2) + [(H, C)]
    assert sum(p.numel() for p in m.parameters()) == sum(i * o + 3 * o for i, o in dims)
    # a checkpoint written by one instance loads into another (both keys name the one tensor)
    c2 = GATConv(9, 16)
    c2.load_state_dict(c.state_dict())
    assert torch.equal(c2.lin_src.weight, c.lin_src.weight) and c2.lin_dst is c2.lin_src


def test_without_self_loops_the_two_transforms_stay_apart():
    from graph_hscn.nn.conv import GATConv
    c = GATConv(3, 4, add_self_loops=False)
    assert c.lin_dst is not c.lin_src
    assert c.lin_src.weight.data_ptr() != c.lin_dst.weight.data_ptr()
    assert sum(1 for _ in c.parameters()) == 5
    t = GATConv((-1, -1), 4, add_self_loops=False)            # the form HSCN builds
    assert t.lin_dst is not t.lin_src


def test_heads_2_raises():
    from graph_hscn.nn.conv import GATConv
    with pytest.raises(NotImplementedError):
        GATConv(3, 4, heads=2)
    with pytest.raises(NotImplementedError):
        GATConv(3, 4, heads=2, add_self_loops=False)


def test_resident_engine_names_the_convolution():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    m = MPNN(CONV_DICT["gat"], ACT_DICT["relu"], 9, 16, 10, 3)
    assert "GATConv" in m.resident_reason()
    assert not m.supported()


def test_new_entries_refuse_bad_arguments_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(64)            # never dereferenced: the refusals below come before any launch
    assert lib.hscn_gat_loop_fwd(None, None, None, None, None, None, None, None, 4, 16, 0.2, 0, None) == -1
    assert lib.hscn_gat_loop_fwd(p, p, p, p, p, None, p, p, -1, 16, 0.2, 0, None) == -1
    assert lib.hscn_gat_loop_fwd(p, p, p, p, p, None, p, p, 4, 0, 0.2, 0, None) == -1
    assert lib.hscn_gat_loop_fwd(p, p, p, p, p, None, p, p, 4, 16, 0.2, 7, None) == -1          # unknown activation
    assert lib.hscn_gat_loop_fwd(p, p, p, p, p, None, p, p, 4, 65, 0.2, 0, None) == -3          # scalar access, > 64
    assert lib.hscn_gat_loop_fwd(p, p, p, p, p, None, p, p, 4, 260, 0.2, 0, None) == -3         # 16-byte access, > 256
    assert lib.hscn_gat_loop_fwd(None, None, None, None, None, None, None, None, 0, 16, 0.2, 0, None) == 0
    assert lib.hscn_gat_loop_bwd_dst(p, p, p, p, p, p, p, None, p, 4, 16, 0.2, None) == -1
    assert lib.hscn_gat_loop_bwd_dst(p, p, p, p, p, p, p, p, p, 4, 65, 0.2, None) == -3
    assert lib.hscn_gat_loop_bwd_src(p, p, p, p, p, p, p, p, p, None, p, p, 4, 16, 0.2, None) == -1
    assert lib.hscn_gat_loop_bwd_src(p, p, p, p, p, p, p, p, p, p, p, p, 4, 65, 0.2, None) == -3


@pytest.mark.parametrize("H", [3, 16])
def test_oracle_identity_against_a_dense_float64_softmax(H):
    """oracle.pyg_ops.GATConv((F, F), H) -- bipartite, no loops -- IS the homogeneous add_self_loops=True operator when
    both transforms hold one weight, x_src = x_dst = x and the edge list is structure.with_self_loops(edge_index, N):
    checked against a dense float64 softmax that knows nothing of edge lists, in float64 (tight) and float32."""
    from graph_hscn.structure import with_self_loops
    from oracle.pyg_ops import GATConv as OGAT
    g = torch.Generator().manual_seed(100 + H)
    N, F = 13, 5
    src = torch.randint(0, N - 2, (40,), generator=g)          # nodes N-2, N-1 stay isolated
    dst = torch.randint(0, N - 2, (40,), generator=g)
    ei = torch.stack([src, dst])
    ei = torch.cat([ei, ei[:, :6],                             # repeated edges
                    torch.tensor([[3, 3, 3, 7], [3, 3, 3, 7]])], 1)   # three loops on node 3, one on node 7
    assert int((ei[0] == ei[1]).sum()) >= 4
    x = torch.randn(N, F, generator=g)
    o = OGAT((F, F), H)
    with torch.no_grad():
        o.lin_dst.weight.copy_(o.lin_src.weight)
        o.bias.copy_(torch.randn(H, generator=g))
    ei_l = with_self_loops(ei, N)
    assert ei_l.shape[1] == int((ei[0] != ei[1]).sum()) + N
    assert torch.equal(ei_l[:, -N:], torch.arange(N).expand(2, -1))
    ref = _dense_gat64(x, o.lin_src.weight.detach(), o.att_src.detach(), o.att_dst.detach(), o.bias.detach(), ei)
    o32 = o(((x, x)), ei_l).detach()
    o64 = o.double()(((x.double(), x.double())), ei_l).detach()
    assert float((o64 - ref).abs().max()) < 1e-12
    assert float((o32.double() - ref).abs().max()) < 1e-5
    # the isolated nodes see only their loop: alpha = 1 / (1 + 1e-16), out = h + bias
    h = x.double() @ o.lin_src.weight.detach().double().t()
    assert torch.allclose(ref[-2:], h[-2:] + o.bias.detach().double(), atol=1e-14)
    # an input loop kept, or the appended loop left out, is a different operator
    kept = torch.cat([ei, torch.arange(N).expand(2, -1)], 1)
    assert float((o.double()((x.double(), x.double()), kept).detach() - ref).abs().max()) > 1e-3
