"""Exphormer without a device: the expander restatement's properties, the union graph's feature-row layout, the
config / constructor validation and the refusals that happen before any launch."""
import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, GPSConfig
from graph_hscn.data import Batch, Data
from graph_hscn.model import gps as gps_model
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import ExphormerAttention
from graph_hscn.structure import EXPH_TYPE_EXPANDER, EXPH_TYPE_LOCAL, ExphormerStructure
from tests import exphormer_oracle as XO


# ---- the expander restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_expander_restatement_is_regular_and_made_of_cycles(n, d):
    ei = XO.expander_edges([n], d, seed=11).numpy()
    assert ei.shape == (2, n * d)
    assert ei.min() >= 0 and ei.max() < n
    assert np.array_equal(np.bincount(ei[0], minlength=n), np.full(n, d))
    assert np.array_equal(np.bincount(ei[1], minlength=n), np.full(n, d))
    for r in range(d // 2):
        fwd, rev = ei[:, 2 * n * r:2 * n * r + n], ei[:, 2 * n * r + n:2 * n * (r + 1)]
        assert np.array_equal(rev, fwd[::-1])                   # the reverses, in the same order
        assert np.array_equal(fwd[1], np.roll(fwd[0], -1))      # edge i ends where edge i + 1 starts
        if n >= 3:                                              # one n-cycle: following it visits every node once
            assert sorted(fwd[0].tolist()) == list(range(n))
            nxt = dict(zip(fwd[0].tolist(), fwd[1].tolist()))
            at, seen = int(fwd[0, 0]), set()
            for _ in range(n):
                seen.add(at)
                at = nxt[at]
            assert len(seen) == n and at == int(fwd[0, 0])
    assert np.array_equal(ei, XO.expander_edges([n], d, seed=11).numpy())
    if n >= 3:
        assert not np.array_equal(ei, XO.expander_edges([n], d, seed=12).numpy())


@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65])
def test_a_graphs_expander_follows_its_id_not_its_place(n, d):
    alone = XO.expander_edges([n], d, seed=3, graph_ids=[5])
    sizes = [4, 1, 7, n, 2]
    batch = XO.expander_edges(sizes, d, seed=3, graph_ids=[9, 8, 7, 5, 6])
    lo = sum(sizes[:3])
    assert torch.equal(batch[:, d * lo:d * (lo + n)] - lo, alone)
    if n >= 3:
        assert not torch.equal(XO.expander_edges(sizes, d, seed=3)[:, d * lo:d * (lo + n)] - lo, alone)


def test_philox_restatement_against_the_published_vectors():
    # Random123 known answers for philox4x32_10: counter 0 / key 0, and all-ones counter words 0, 1 with key words
    # all ones -- the second has counter words 2, 3 non-zero, so only the first is within this restatement's reach;
    # it is pinned together with the copy in tests/test_gpu_exact_edges.py
    from tests.test_gpu_exact_edges import philox4x32_10
    assert int(XO.philox_word0(np.array([0], dtype=np.uint64), 0)[0]) == 0x6627E8D5
    ctr = np.array([0, 1, 2 ** 32 + 5, 2 ** 63 + 12345], dtype=np.uint64)
    seed = 0x1234567887654321
    words = np.stack([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.zeros(4, np.uint64), np.zeros(4, np.uint64)], 1)
    ref = philox4x32_10(words, (seed & 0xFFFFFFFF, seed >> 32))[:, 0].astype(np.uint64)
    assert np.array_equal(XO.philox_word0(ctr, seed), ref)


# ---- the union graph -----------------------------------------------------------------------------------------------
def _two_graphs(edge_attr):
    g0 = Data(x=torch.zeros(3, 2), edge_index=torch.tensor([[0, 1, 2, 2], [1, 0, 0, 2]]))
    g1 = Data(x=torch.zeros(2, 2), edge_index=torch.tensor([[1, 0], [0, 1]]))
    if edge_attr:
        g0.edge_attr, g1.edge_attr = torch.zeros(4, 3), torch.zeros(2, 3)
    return Batch.from_data_list([g0, g1])


@pytest.mark.parametrize("nv", [0, 2])
@pytest.mark.parametrize("edge_attr", [False, True])
def test_erow_and_type_layout_on_a_hand_written_batch(edge_attr, nv):
    b = _two_graphs(edge_attr)
    ex = XO.expander_edges([3, 2], 2, seed=0)
    st = ExphormerStructure(b.edge_index, b.batch, 2, ex, nv, add_local_edges=True, edge_features=edge_attr)
    N, El = 5, (6 if edge_attr else 0)
    assert (st.num_nodes, st.num_graphs, st.num_rows, st.num_types, st.num_edge_rows) == (N, 2, N + 2 * nv, 2 + 2 * nv, El)
    assert st.num_edges == 6 + 10 + 2 * N * nv and st.erow.dtype == torch.int32
    ei, erow = st.edge_index, st.erow.tolist()
    # local block: its own rows with features, type 0 without
    assert torch.equal(ei[:, :6], b.edge_index)
    assert erow[:6] == (list(range(6)) if edge_attr else [El + EXPH_TYPE_LOCAL] * 6)
    # expander block
    assert torch.equal(ei[:, 6:16], ex) and erow[6:16] == [El + EXPH_TYPE_EXPANDER] * 10
    if nv:
        graph_of = [0, 0, 0, 1, 1]
        n2v, v2n = ei[:, 16:16 + N * nv], ei[:, 16 + N * nv:]
        for i in range(N):
            for t in range(nv):
                virt = N + graph_of[i] * nv + t
                assert n2v[:, i * nv + t].tolist() == [i, virt] and v2n[:, i * nv + t].tolist() == [virt, i]
                assert erow[16 + i * nv + t] == El + 2 + t
                assert erow[16 + N * nv + i * nv + t] == El + 2 + nv + t
    # and the restatement says the same
    uei, uerow, uEl, uT, urows = XO.union_graph(b.edge_index, b.batch, 2, ex, nv, True, edge_attr)
    assert torch.equal(uei, ei) and uerow.tolist() == erow and (uEl, uT, urows) == (El, st.num_types, st.num_rows)
    # without the local edges nothing names a per-edge row
    st2 = ExphormerStructure(b.edge_index, b.batch, 2, ex, nv, add_local_edges=False, edge_features=edge_attr)
    assert st2.num_edge_rows == 0 and st2.num_edges == 10 + 2 * N * nv and st2.erow[:10].tolist() == [1] * 10


def test_structure_refuses_more_than_four_virtual_nodes():
    b = _two_graphs(False)
    with pytest.raises(ValueError, match="num_virtual_nodes"):
        ExphormerStructure(b.edge_index, b.batch, 2, None, 5)


# ---- constants and envelopes (host functions of the library) -------------------------------------------------------
def test_python_constants_are_the_librarys():
    L = _hip.lib()
    assert L.hscn_expander_max_nodes() == Fh.EXPANDER_MAX_NODES == 2048
    assert L.hscn_expander_max_degree() == Fh.EXPANDER_MAX_DEGREE == 32
    assert L.hscn_exph_max_types() == 2 + 2 * Fh.EXPH_MAX_VIRTUAL_NODES
    assert L.hscn_exph_attn_long_row() == L.hscn_edge_attn_long_row()
    assert L.hscn_exph_attn_chunk() == L.hscn_edge_attn_chunk()
    assert L.hscn_exph_type_long_row() >= L.hscn_exph_type_chunk() >= 1
    assert Fh.exph_attn_supported(8, 64) and Fh.exph_attn_supported(1, 512) and Fh.exph_attn_supported(2, 70)
    assert not Fh.exph_attn_supported(1, 513) and not Fh.exph_attn_supported(0, 4)
    assert L.hscn_abi_version() == 24


def test_entry_points_refuse_before_any_launch():
    L = _hip.lib()
    one = 1                                        # (a non-NULL address that is never dereferenced)
    assert L.hscn_expander_build(one, None, 4, 1, 3, 0, 8, one, one, None) == -1          # odd degree
    assert L.hscn_expander_build(one, None, 4, 1, 0, 0, 8, one, one, None) == -1
    assert L.hscn_expander_build(one, None, 4, 1, 34, 0, 8, one, one, None) == -3         # degree > 32
    assert L.hscn_expander_build(one, None, 4, 1, 2, 0, 2049, one, one, None) == -3       # beyond the envelope
    assert L.hscn_expander_build(None, None, 4, 1, 2, 0, 8, one, one, None) == -1
    assert L.hscn_expander_build(one, None, 0, 0, 2, 0, 8, None, one, None) == 0
    assert L.hscn_exph_attn_fwd(*([one] * 11), 4, 4, 0, 2, 1, 513, one, None) == -3
    assert L.hscn_exph_attn_fwd(*([one] * 11), 4, 4, 0, 11, 1, 16, one, None) == -3       # more than 10 types
    assert L.hscn_exph_attn_fwd(*([one] * 7), None, one, one, one, 4, 4, 2, 2, 1, 16, one, None) == -1   # El without e_edge
    assert L.hscn_exph_attn_bwd_type(*([one] * 11), 4, 4, 2, 1, 16, one, one, 0, None) == -2              # short workspace
    assert L.hscn_exph_type_workspace_bytes(130, 4, 2, 8) == (130 // L.hscn_exph_type_chunk() + 4) * 16 * 4


# ---- config and constructor validation -------------------------------------------------------------------------------
def test_config_validation():
    cfg = GPSConfig("relu", global_model="exphormer")
    assert (cfg.expander_degree, cfg.num_virtual_nodes, cfg.add_local_edges, cfg.expander_seed) == (6, 1, True, 0)
    assert GPSConfig("relu").global_model == "attention"
    with pytest.raises(ValueError, match="expander_degree"):
        GPSConfig("relu", global_model="exphormer", expander_degree=5)
    with pytest.raises(ValueError, match="expander_degree"):
        GPSConfig("relu", global_model="exphormer", expander_degree=34)
    with pytest.raises(ValueError, match="num_virtual_nodes"):
        GPSConfig("relu", global_model="exphormer", num_virtual_nodes=5)
    with pytest.raises(ValueError, match="global_model"):
        GPSConfig("relu", global_model="performer")
    with pytest.raises(ValueError, match=r"exphormer.*attn_bias|attn_bias.*exphormer"):
        GPSConfig("relu", global_model="exphormer", attn_bias="spd")


def test_model_constructor_validation():
    kw = dict(num_features=9, hidden_channels=16, num_classes=3, num_layers=1, num_heads=4, local_conv=None)
    with pytest.raises(ValueError, match="expander_degree"):
        GPS(**kw, global_model="exphormer", expander_degree=3)
    with pytest.raises(ValueError, match="num_virtual_nodes"):
        GPS(**kw, global_model="exphormer", num_virtual_nodes=5)
    with pytest.raises(ValueError, match=r"exphormer.*attn_bias"):
        GPS(**kw, global_model="exphormer", attn_bias="spd")
    with pytest.raises(ValueError, match="global_model"):
        GPS(**kw, global_model="dense")
    with pytest.raises(ValueError, match="num_virtual_nodes"):
        ExphormerAttention(16, 4, 5)
    m = build_gps(GPSConfig("relu", local_conv_type=None, hidden_channels=16, num_layers=1, global_model="exphormer",
                            expander_degree=4, num_virtual_nodes=2, expander_seed=7), 9, 3)
    assert (m.global_model, m.expander_degree, m.num_virtual_nodes, m.expander_seed) == ("exphormer", 4, 2, 7)
    assert tuple(m.virt_node_emb.weight.shape) == (2, 16) and tuple(m.edge_type_emb.weight.shape) == (6, 16)
    assert tuple(m.layers[0].attn.E.weight.shape) == (16, 16) and m.layers[0].attn.Q.bias is None


def test_a_default_gps_has_the_state_dict_of_before():
    m = GPS(9, 16, 3, 1, 4, "gine")
    assert list(m.state_dict().keys()) == [
        "node_encoder.weight", "node_encoder.bias", "layers.0.conv.eps", "layers.0.conv.nn.0.weight",
        "layers.0.conv.nn.0.bias", "layers.0.conv.nn.2.weight", "layers.0.conv.nn.2.bias", "layers.0.conv.lin.weight",
        "layers.0.conv.lin.bias", "layers.0.attn.in_proj_weight", "layers.0.attn.in_proj_bias",
        "layers.0.attn.out_proj.weight", "layers.0.attn.out_proj.bias", "layers.0.norm1_local.weight",
        "layers.0.norm1_local.bias", "layers.0.norm1_attn.weight", "layers.0.norm1_attn.bias",
        "layers.0.ff_linear1.weight", "layers.0.ff_linear1.bias", "layers.0.ff_linear2.weight",
        "layers.0.ff_linear2.bias", "layers.0.norm2.weight", "layers.0.norm2.bias", "lin_1.weight", "lin_1.bias",
        "lin_2.weight", "lin_2.bias"]
    assert m.global_model == "attention" and m.resident_reason() == gps_model.RESIDENT_REASON


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _cpu_batch():
    g = torch.Generator().manual_seed(0)
    graphs = [Data(x=torch.randn(n, 9, generator=g), edge_index=torch.randint(0, n, (2, 2 * n), generator=g),
                   y=torch.zeros(1, 3)) for n in (5, 7)]
    return Batch.from_data_list(graphs)


def test_cpu_tensors_are_refused():
    b = _cpu_batch()
    with pytest.raises(RuntimeError, match="HIP device tensors only"):
        Fh.expander_edges(b.ptr32, 2, 0, max_nodes=b.max_nodes)
    ex = XO.expander_edges([5, 7], 2, seed=0)
    st = ExphormerStructure(b.edge_index, b.batch, 2, ex, 1, True, False)
    q = torch.randn(st.num_rows, 16)
    with pytest.raises(RuntimeError, match="HIP device tensors only"):
        Fh.ExphormerAttentionFn.apply(q, q, q, None, torch.randn(4, 16), st, 4)
    with pytest.raises(TypeError, match="float32"):
        Fh.ExphormerAttentionFn.apply(q.double(), q, q, None, torch.randn(4, 16), st, 4)
    with pytest.raises(ValueError, match="edge types"):
        Fh.ExphormerAttentionFn.apply(q, q, q, None, torch.randn(5, 16), st, 4)
    with pytest.raises(ValueError, match="rows"):
        Fh.ExphormerAttentionFn.apply(q[:-1], q[:-1], q[:-1], None, torch.randn(4, 16), st, 4)
    with pytest.raises(ValueError, match="degree"):
        Fh.expander_edges(b.ptr32, 3, 0, max_nodes=b.max_nodes)
    with pytest.raises(ValueError, match="envelope"):
        Fh.expander_edges(b.ptr32, 2, 0, max_nodes=2049)


def test_the_resident_engine_refuses_the_model_with_its_own_reason():
    m = GPS(9, 16, 3, 1, 4, None, ACT_DICT["relu"], global_model="exphormer")
    assert m.layered_only and not m.supported()
    assert "Exphormer" in m.resident_reason() and m.resident_reason() == gps_model.EXPHORMER_RESIDENT_REASON
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="Exphormer's sparse attention"):
        m(_cpu_batch())
