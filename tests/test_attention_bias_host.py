"""Shortest-path attention bias, everything that answers without a GPU: the oracle's BFS against an independent
Floyd-Warshall restatement, the C ABI's exports, envelopes and argument checks (all before any launch), ``GPSConfig``,
the refusals of the Python layers by their messages, the ``state_dict`` keys with and without the table and the order
of the initialisation draws."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import GPSConfig
from graph_hscn.data import Batch, Data
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import MultiheadSelfAttention
from graph_hscn.nn.gps import GPSLayer
from tests import attention_bias_oracle as BO

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
_BUF = ctypes.create_string_buffer(512)
_HERE = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte aligned host address standing in for a pointer


def _floyd_warshall(n, edge_index, max_dist):
    """min(d, max_dist) by the all-pairs recurrence d[i][j] = min(d[i][j], d[i][k] + d[k][j]): no search, no frontier."""
    INF = 10 ** 9
    d = [[0 if i == j else INF for j in range(n)] for i in range(n)]
    for a, b in zip(edge_index[0].tolist(), edge_index[1].tolist()):
        if a != b:
            d[a][b] = 1
    for k in range(n):
        dk = d[k]
        for i in range(n):
            dik = d[i][k]
            if dik < INF:
                di = d[i]
                for j in range(n):
                    if dik + dk[j] < di[j]:
                        di[j] = dik + dk[j]
    return torch.tensor([[min(v, max_dist) for v in row] for row in d], dtype=torch.uint8).reshape(n, n)


@pytest.mark.parametrize("max_dist", [1, 5, 63])
def test_oracle_bfs_equals_floyd_warshall_on_the_edge_case_graphs(max_dist):
    graphs = BO.edge_case_graphs()
    ei, ptr, eptr = BO.collate(graphs)
    got = BO.bfs_buckets(ei, ptr, max_dist, eptr)
    assert len(got) == len(graphs)
    for (n, e), m in zip(graphs, got):
        assert m.dtype == torch.uint8 and m.shape == (n, n)
        assert torch.equal(m, _floyd_warshall(n, e, max_dist)), n
    if max_dist == 5:
        cyc, path = got[3], got[4]
        assert cyc.tolist() == [[0, 1, 2], [2, 0, 1], [1, 2, 0]]              # directed: d(i, j) != d(j, i)
        assert path[0].tolist() == [0, 1, 2, 3, 4] + [5] * 7                  # the cap is crossed
        assert got[1].tolist() == [[0 if i == j else 5 for j in range(5)] for i in range(5)]
        assert int(got[2][0, 4]) == 5 and int(got[2][4, 6]) == 2              # unreachable / inside a component
    # without eptr an edge belongs to its source's graph: the same answer
    assert all(torch.equal(a, b) for a, b in zip(got, BO.bfs_buckets(ei, ptr, max_dist)))


def test_exports_and_envelopes():
    lib = _hip.lib()
    for name in ("hscn_attention_bias_fwd", "hscn_attention_bias_bwd_q", "hscn_attention_bias_bwd_kv",
                 "hscn_attention_bias_supported", "hscn_spd_buckets", "hscn_spd_supported"):
        assert hasattr(lib, name) and name in _hip.exported_symbols()
    assert lib.hscn_abi_version() == 24
    # buckets: 1 .. 64; heads and dh: the unbiased operator's envelope
    for nb, ok in ((0, 0), (1, 1), (2, 1), (64, 1), (65, 0), (-1, 0)):
        assert lib.hscn_attention_bias_supported(4, 16, nb) == ok, nb
    for heads, dh in ((1, 4), (8, 64), (128, 4), (1, 2), (1, 68), (129, 4), (2, 6), (0, 8)):
        assert lib.hscn_attention_bias_supported(heads, dh, 21) == lib.hscn_attention_supported(heads, dh)
    # max_dist: 1 .. 63; nodes: three bitsets of n x ceil(n / 32) words and 1 KB within 160 KB
    for md, ok in ((0, 0), (1, 1), (63, 1), (64, 0), (-3, 0)):
        assert lib.hscn_spd_supported(100, md) == ok, md
    assert lib.hscn_spd_supported(512, 20) == 1 and lib.hscn_spd_supported(0, 20) == 1
    assert lib.hscn_spd_supported(-1, 20) == 0
    largest = max(n for n in range(512, 1025) if lib.hscn_spd_supported(n, 20))
    need = lambda n: 3 * n * -(-n // 32) * 4 + 1024
    assert need(largest) <= 160 * 1024 < need(largest + 1)
    assert largest == 646 and Fh.spd_supported(646, 63) and not Fh.spd_supported(647, 63)
    assert (Fh.SPD_MIN_DIST, Fh.SPD_MAX_DIST, Fh.ATTN_MAX_BUCKETS) == (1, 63, 64)


def _spd(ei, ptr, eptr, sptr, N, E, B, total, mn, md, bucket, flag):
    return _hip.lib().hscn_spd_buckets(ei, ptr, eptr, sptr, N, E, B, total, mn, md, bucket, flag, None)


def _fwd(p, N, B, total, mn, heads, dh, nb, qkv=0, out=0):
    q = p if qkv == 0 else qkv
    o = p if out == 0 else out
    return _hip.lib().hscn_attention_bias_fwd(q, p, p, p, p, N, B, total, mn, heads, dh, nb, o, p, p, None)


def _bwd_q(p, N, B, total, mn, heads, dh, nb, g_qkv=0, g_table=0, work=0, floats=1 << 40):
    a = [p if v == 0 else v for v in (g_qkv, g_table, work)]
    return _hip.lib().hscn_attention_bias_bwd_q(p, p, p, p, p, p, p, p, N, B, total, mn, heads, dh, nb, a[0], p, a[1],
                                                a[2], floats, p, None)


def _bwd_kv(p, N, B, total, mn, heads, dh, nb):
    return _hip.lib().hscn_attention_bias_bwd_kv(p, p, p, p, p, p, p, p, N, B, total, mn, heads, dh, nb, p, p, None)


def test_argument_checks_answer_before_any_launch():
    H = _HERE
    # the bucket kernel: negative sizes, the envelope, nothing to do, null pointers
    assert _spd(H, H, H, H, -1, 0, 1, 4, 4, 5, H, H) == BADARG
    assert _spd(H, H, H, H, 4, -1, 1, 4, 4, 5, H, H) == BADARG
    assert _spd(H, H, H, H, 4, 0, 1, -4, 4, 5, H, H) == BADARG
    assert _spd(H, H, H, H, 1 << 31, 0, 1, 4, 4, 5, H, H) == BADARG
    for mn, md in ((647, 5), (4, 0), (4, 64), (100000, 5)):
        assert _spd(H, H, H, H, 4, 0, 1, 16, mn, md, H, H) == UNSUPPORTED, (mn, md)
    assert _spd(None, None, None, None, 0, 0, 3, 0, 4, 5, None, None) == 0
    assert _spd(None, None, None, None, 5, 0, 0, 0, 4, 5, None, None) == 0
    for k in (1, 2, 3, 5):                                   # ptr32, eptr32, spd_ptr, flag
        args = [H] * 6
        args[k] = None
        assert _spd(args[0], args[1], args[2], args[3], 4, 0, 1, 16, 4, 5, args[4], args[5]) == BADARG, k
    assert _spd(None, H, H, H, 4, 3, 1, 16, 4, 5, H, H) == BADARG            # edges without edge_index
    assert _spd(H, H, H, H, 4, 0, 1, 16, 4, 5, None, H) == BADARG            # room asked for, no bucket
    # the biased operator
    assert _fwd(H, -1, 1, 16, 4, 1, 4, 6) == BADARG and _fwd(H, 4, 1, -1, 4, 1, 4, 6) == BADARG
    for heads, dh, nb in ((1, 2, 6), (1, 68, 6), (129, 4, 6), (2, 8, 0), (2, 8, 65)):
        assert _fwd(H, 4, 1, 16, 4, heads, dh, nb) == UNSUPPORTED, (heads, dh, nb)
        assert _bwd_q(H, 4, 1, 16, 4, heads, dh, nb) == UNSUPPORTED
        assert _bwd_kv(H, 4, 1, 16, 4, heads, dh, nb) == UNSUPPORTED
    assert _fwd(None, 0, 3, 0, 4, 1, 4, 6) == 0 and _bwd_kv(None, 0, 0, 0, 0, 2, 8, 6) == 0
    assert _fwd(None, 4, 1, 16, 4, 1, 4, 6) == BADARG and _bwd_kv(None, 4, 1, 16, 4, 1, 4, 6) == BADARG
    assert _fwd(H, 4, 1, 16, 4, 1, 4, 6, qkv=H + 4) == BADARG and _fwd(H, 4, 1, 16, 4, 1, 4, 6, out=H + 8) == BADARG
    # bwd_q: something must be asked for; a table gradient needs its workspace, large enough
    assert _bwd_q(H, 4, 1, 16, 4, 1, 4, 6, g_qkv=None, g_table=None) == BADARG
    assert _bwd_q(H, 4, 1, 16, 4, 1, 4, 6, work=None) == BADARG
    tile = _hip.lib().hscn_attention_tile()
    need = 3 * -(-(tile + 1) // tile) * 2 * 6                # B tiles heads buckets
    assert _bwd_q(H, 4, 3, 16, tile + 1, 2, 8, 6, floats=need - 1) == WORKSPACE
    assert _bwd_q(None, 4, 1, 16, 4, 1, 4, 6, g_qkv=H, g_table=None, work=None) == BADARG      # null inputs


def test_gps_config_validation():
    cfg = GPSConfig("relu")
    assert cfg.attn_bias is None and cfg.spd_max_dist == 20
    cfg = GPSConfig("relu", attn_bias="spd", spd_max_dist=7)
    m = build_gps(cfg, 9, 10)
    assert m.attn_bias == "spd" and m.spd_max_dist == 7
    assert all(layer.attn.spd_buckets == 8 and tuple(layer.attn.spd_bias.weight.shape) == (8, cfg.num_heads)
               for layer in m.layers)
    assert build_gps(GPSConfig("relu"), 9, 10).attn_bias is None
    GPSConfig("relu", attn_bias="spd", spd_max_dist=1)
    GPSConfig("relu", attn_bias="spd", spd_max_dist=63)
    for bad in ("SPD", "dense", "graphormer", 1):
        with pytest.raises(ValueError, match="attn_bias must be 'spd' or None"):
            GPSConfig("relu", attn_bias=bad)
    for bad in (0, 64, -1, 2.5, True):
        with pytest.raises(ValueError, match=r"spd_max_dist must be an integer in \[1, 63\]"):
            GPSConfig("relu", attn_bias="spd", spd_max_dist=bad)
    with pytest.raises(ValueError, match="attn_bias must be 'spd' or None"):
        GPS(9, 16, 10, 2, attn_bias="dense")
    with pytest.raises(ValueError, match=r"spd_max_dist must be in \[1, 63\]"):
        GPS(9, 16, 10, 2, attn_bias="spd", spd_max_dist=64)


def _cycle_batch(n):
    e = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    return Batch.from_data_list([Data(x=torch.zeros(n, 3), edge_index=e)])


def test_refusals_by_name():
    x = torch.randn(5, 16)
    ptr32 = torch.tensor([0, 5], dtype=torch.int32)
    spd6 = Fh.SPDBuckets(torch.zeros(25, dtype=torch.uint8), torch.tensor([0, 25]), 5, 5)
    # spd= without spd_buckets, and spd_buckets without (or with the wrong) spd=
    with pytest.raises(ValueError, match="has no shortest-path bias table"):
        MultiheadSelfAttention(16, 4)(x, ptr32=ptr32, max_nodes=5, spd=spd6)
    with pytest.raises(ValueError, match="has no shortest-path bias table"):
        GPSLayer(16, None, 4)(x, None, ptr32=ptr32, max_nodes=5, spd=spd6)
    att = MultiheadSelfAttention(16, 4, spd_buckets=8)
    with pytest.raises(ValueError, match="needs spd="):
        att(x, ptr32=ptr32, max_nodes=5)
    with pytest.raises(ValueError, match=r"max_dist \+ 1 = 6 buckets.*spd_buckets = 8"):
        att(x, ptr32=ptr32, max_nodes=5, spd=spd6)
    # the dense tensor keyword stays refused, with or without a table
    for mod in (MultiheadSelfAttention(16, 4), att):
        with pytest.raises(NotImplementedError, match="attn_bias"):
            mod(x, ptr32=ptr32, max_nodes=5, attn_bias=torch.zeros(5, 5))
    for bad in (0, 1, 65):
        with pytest.raises(ValueError, match="spd_buckets must be max_dist"):
            MultiheadSelfAttention(16, 4, spd_buckets=bad)
    # max_dist outside [1, 63]
    b = _cycle_batch(5)
    for bad in (0, 64, -2):
        with pytest.raises(ValueError, match=r"max_dist must be in \[1, 63\]"):
            Fh.shortest_path_buckets(b, bad)
    # a batch beyond the envelope: refused on the host, before the device is looked at
    with pytest.raises(ValueError, match="647 nodes is outside the kernel's envelope"):
        Fh.shortest_path_buckets(_cycle_batch(647), 20)
    with pytest.raises(ValueError, match="outside the kernel's envelope"):
        Fh.shortest_path_buckets((b.edge_index, b.ptr32, b.eptr32, 5000), 20, sizes=[5])
    # node counts come from the host: to_device takes them from ptr, and shares one cache dict with the loader's batch
    from graph_hscn.train import batching
    moved = batching.to_device(None, b, "cpu")
    assert moved._host_sizes == (5,) and moved._spd_cache is b._spd_cache == {}
    assert batching.to_device(None, moved, "cpu")._spd_cache is b._spd_cache
    assert set(b.keys()) == set(moved.keys())
    with pytest.raises(ValueError, match="node count on the host"):
        Fh.shortest_path_buckets((b.edge_index, b.ptr32, b.eptr32, 5), 20)
    with pytest.raises(ValueError, match="2 sizes for 1 graphs"):
        Fh.shortest_path_buckets(b, 20, sizes=[2, 3])
    with pytest.raises(ValueError, match="carries no eptr32"):
        Fh.shortest_path_buckets(SimpleNamespace(edge_index=b.edge_index, ptr32=b.ptr32, max_nodes=5), 20)
    with pytest.raises(ValueError, match="node count on the host"):
        Fh.shortest_path_buckets(_cycle_batch(5), 20)         # a batch nobody moved
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
        Fh.shortest_path_buckets(moved, 20)
    # the operator: the table's shape, the spd's type, no CPU fallback
    with pytest.raises(TypeError, match="SPDBuckets"):
        Fh.BiasedSelfAttentionFn.apply(torch.randn(5, 48), torch.zeros(6, 4), None, ptr32, 5, 4)
    with pytest.raises(ValueError, match=r"table must be \[6, 4\]"):
        Fh.BiasedSelfAttentionFn.apply(torch.randn(5, 48), torch.zeros(8, 4), spd6, ptr32, 5, 4)
    with pytest.raises(ValueError, match="envelope"):
        Fh.BiasedSelfAttentionFn.apply(torch.randn(5, 24), torch.zeros(6, 4), spd6, ptr32, 5, 4)      # head width 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fh.BiasedSelfAttentionFn.apply(torch.randn(5, 48), torch.zeros(6, 4), spd6, ptr32, 5, 4)
    # the model on a CPU batch: the bucket build refuses, nothing falls back
    graphs = make_dataset("peptides_func", 2, seed=0)
    with pytest.raises(RuntimeError, match="shortest_path_buckets takes HIP device tensors only"):
        GPS(9, 16, 10, 1, 4, None, attn_bias="spd")(batching.to_device(None, Batch.from_data_list(graphs), "cpu"))


def test_state_dict_keys_with_and_without_the_table():
    torch.manual_seed(0)
    plain = GPS(9, 16, 10, 2, 4, "gcn")
    keys = list(plain.state_dict())
    assert not any("spd" in k for k in keys)
    assert [k for k in keys if ".attn." in k and k.startswith("layers.0.")] == [
        "layers.0.attn.in_proj_weight", "layers.0.attn.in_proj_bias", "layers.0.attn.out_proj.weight",
        "layers.0.attn.out_proj.bias"]
    torch.manual_seed(0)
    assert list(GPS(9, 16, 10, 2, 4, "gcn", attn_bias=None, spd_max_dist=7).state_dict()) == keys
    biased = GPS(9, 16, 10, 2, 4, "gcn", attn_bias="spd", spd_max_dist=7)
    extra = [f"layers.{i}.attn.spd_bias.weight" for i in range(2)]
    assert sorted(biased.state_dict()) == sorted(keys + extra)
    assert all(tuple(biased.state_dict()[k].shape) == (8, 4) for k in extra)
    # a module without the table is torch.nn.MultiheadAttention's, key for key; with it, one key more, last
    a = list(MultiheadSelfAttention(16, 4).state_dict())
    assert a == list(torch.nn.MultiheadAttention(16, 4).state_dict())
    assert list(MultiheadSelfAttention(16, 4, spd_buckets=21).state_dict()) == a + ["spd_bias.weight"]
    assert list(GPSLayer(16, None, 4).state_dict()) == [k for k in GPSLayer(16, None, 4, spd_buckets=21).state_dict()
                                                        if "spd" not in k]


@pytest.mark.parametrize("D,heads", [(16, 4), (64, 1)])
def test_the_table_is_drawn_after_the_existing_draws(D, heads):
    torch.manual_seed(11)
    plain = MultiheadSelfAttention(D, heads).state_dict()
    torch.manual_seed(11)
    biased = MultiheadSelfAttention(D, heads, spd_buckets=21).state_dict()
    for k in ("in_proj_weight", "out_proj.weight", "in_proj_bias", "out_proj.bias"):
        assert torch.equal(plain[k], biased[k]), k
    w = biased["spd_bias.weight"]
    assert tuple(w.shape) == (21, heads) and 0.0 < float(w.std()) < 0.06 and float(w.abs().max()) < 0.2   # normal(0, 0.02)
    # the model: the same seed gives the same weights wherever a key exists in both
    torch.manual_seed(3)
    a = GPS(9, 16, 10, 1, 4, None).state_dict()
    torch.manual_seed(3)
    b = GPS(9, 16, 10, 1, 4, None, attn_bias="spd").state_dict()
    assert torch.equal(a["layers.0.attn.in_proj_weight"], b["layers.0.attn.in_proj_weight"])
    assert torch.equal(a["layers.0.attn.out_proj.weight"], b["layers.0.attn.out_proj.weight"])
