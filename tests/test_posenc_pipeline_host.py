"""Host side of the positional-encoding stage: the batch containers' per-node extras and ``to_data_list``,
``get_each_data_from_batch`` / ``pre_transform_in_memory``, the ABI entries of the one-launch SignNet encoder
(refusals before any launch, both sides of every envelope edge), and the algebra the kernel rests on -- everything in
front of the encoder's one ReLU is linear in a channel's scalar input -- against the oracle in float64.  No GPU needed."""
import ctypes

import pytest
import torch

from oracle import signnet as OS


def _ragged(extras, target):
    """Five ragged graphs: a 1-node graph, a graph with no edges, repeated / one-way edges."""
    from graph_hscn.data import Data
    g = torch.Generator().manual_seed(7)
    sizes = [5, 1, 4, 7, 3]
    out = []
    for i, n in enumerate(sizes):
        if n == 1 or i == 2:
            ei = torch.zeros(2, 0, dtype=torch.long)
        else:
            ei = torch.randint(0, n, (2, 2 * n + i), generator=g)
        d = Data(x=torch.randn(n, 3, generator=g), edge_index=ei, num_nodes=n)
        if target == "rows":
            d.y = torch.randn(1, 4, generator=g)
        elif target == "class":
            d.y = torch.randint(0, 6, (1,), generator=g)
        elif target == "node":
            d.y = torch.randint(0, 6, (n,), generator=g)
        if extras:
            d.eigvecs_sn = torch.randn(n, 6, generator=g)
            d.eigvecs_sn[:, min(n, 6):] = float("nan")
            d.eigvals_sn = torch.randn(n, 6, 1, generator=g)
        out.append(d)
    return out


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(torch.nan_to_num(a.double(), nan=12345.0), torch.nan_to_num(b.double(), nan=12345.0))
    return a == b


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("target", ["rows", "class", "node", "none"])
def test_from_data_list_to_data_list_round_trip(extras, target):
    from graph_hscn.data import Batch
    graphs = _ragged(extras, target)
    b = Batch.from_data_list(graphs)
    want_keys = {"x", "edge_index", "y", "edge_weight", "num_nodes", "batch", "ptr", "num_graphs", "ptr32", "eptr32",
                 "max_nodes", "max_edges"} | ({"eigvecs_sn", "eigvals_sn"} if extras else set())
    assert set(b.keys()) == want_keys                       # without extras: exactly the keys of the batch of before
    if extras:
        assert b.eigvecs_sn.shape == (20, 6) and b.eigvals_sn.shape == (20, 6, 1)
        assert _same(b.eigvecs_sn, torch.cat([g.eigvecs_sn for g in graphs], 0))
    back = b.to_data_list()
    assert len(back) == len(graphs)
    for g, h in zip(graphs, back):
        assert h.num_nodes == g.num_nodes
        assert _same(h.x, g.x) and _same(h.edge_index, g.edge_index)
        if target == "none":
            assert h.y is None
        else:
            assert _same(h.y, g.y)
        if extras:
            assert _same(h.eigvecs_sn, g.eigvecs_sn) and _same(h.eigvals_sn, g.eigvals_sn)
        else:
            assert "eigvecs_sn" not in h
    b2 = Batch.from_data_list(back)
    assert set(b2.keys()) == set(b.keys())
    for k in b.keys():
        assert _same(b2._d[k], b._d[k]), k


def test_extras_need_every_graph_and_the_node_count():
    from graph_hscn.data import Batch
    graphs = _ragged(True, "rows")
    del graphs[3]._d["eigvals_sn"]                          # one graph without it: not carried
    graphs[0].note = torch.zeros(2)                         # not per node
    b = Batch.from_data_list(graphs)
    assert "eigvecs_sn" in b and "eigvals_sn" not in b and "note" not in b


def test_get_each_data_from_batch_and_edge_weights():
    from graph_hscn.data import Batch
    from graph_hscn.train import get_each_data_from_batch
    graphs = _ragged(True, "rows")
    for g in graphs:
        g.edge_weight = torch.rand(g.edge_index.size(1))
    batches = [Batch.from_data_list(graphs[:2]), Batch.from_data_list(graphs[2:])]
    flat = get_each_data_from_batch(batches)
    assert len(flat) == 5
    for g, h in zip(graphs, flat):
        assert _same(h.x, g.x) and _same(h.edge_index, g.edge_index) and _same(h.edge_weight, g.edge_weight)
        assert _same(h.eigvecs_sn, g.eigvecs_sn)
    assert get_each_data_from_batch([]) == []


def test_pre_transform_in_memory():
    from graph_hscn.transform import pre_transform_in_memory
    from graph_hscn.transform.pre_transform import pre_transform_in_memory as same
    assert same is pre_transform_in_memory
    graphs = _ragged(False, "rows")
    assert pre_transform_in_memory(graphs, None) is graphs

    def double_or_drop(g):
        if g.num_nodes == 1:
            return None
        g.x = g.x * 2
        return g

    xs = [g.x.clone() for g in graphs]
    kept = [g for g in graphs if g.num_nodes != 1]
    assert pre_transform_in_memory(graphs, double_or_drop, show_progress=False) is None
    assert len(graphs) == 4 and all(a is b for a, b in zip(graphs, kept))      # in place, the 1-node graph removed
    assert torch.equal(graphs[0].x, xs[0] * 2) and torch.equal(graphs[1].x, xs[2] * 2)


def test_abi_version_and_new_symbols():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert lib.hscn_abi_version() == 24 == _hip.ABI_VERSION
    assert {"hscn_signnet_supported", "hscn_signnet_encode"} <= set(_hip.exported_symbols())


# model, use_bn, F, K, hidden, phi_out, layers, post_layers, dim_pe, dim_x, max_n, max_e
_OK = dict(model=0, use_bn=0, F=9, K=10, hidden=32, phi_out=4, layers=1, post_layers=1, dim_pe=8, dim_x=8, max_n=444,
           max_e=2664)


def _sup(**kw):
    from graph_hscn import _hip
    a = dict(_OK, **kw)
    return _hip.lib().hscn_signnet_supported(*[a[k] for k in _OK])


def test_signnet_supported_at_both_sides_of_each_edge():
    assert _sup() == 1                                       # Peptides' largest graph at the default widths
    assert _sup(max_n=500, max_e=3000) == 1                  # PascalVOC-SP's
    assert _sup(model=1) == 0 and _sup(use_bn=1) == 0
    for name, lo, hi in [("F", 1, 1024), ("dim_x", 1, 1024), ("K", 1, 64), ("hidden", 1, 64), ("phi_out", 1, 64),
                         ("dim_pe", 1, 64), ("layers", 1, 8), ("post_layers", 1, 8)]:
        small = dict(max_n=16, max_e=32)
        assert _sup(**{name: lo}, **small) == 1 and _sup(**{name: lo - 1}, **small) == 0, name
        assert _sup(**{name: hi}, **small) == 1 and _sup(**{name: hi + 1}, **small) == 0, name
    assert _sup(max_n=0, max_e=0) == 1 and _sup(max_n=-1) == 0 and _sup(max_e=-1) == 0
    # the LDS edge: the largest node count the layout takes at these widths, and one more
    lo, hi = 500, 4000
    assert _sup(max_n=lo, max_e=0) == 1 and _sup(max_n=hi, max_e=0) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _sup(max_n=mid, max_e=0) else (lo, mid)
    assert _sup(max_n=lo, max_e=0) == 1 and _sup(max_n=lo + 1, max_e=0) == 0
    # by arithmetic (csrc/signnet.hip: sn_layout): two tables of 3 x 32, rowptr, two scalar fields, two [n, 10]
    # channel fields, two 32 x 32 tiles and [n, 32] words of c, every array rounded up to four words
    up4 = lambda v: (v + 3) & ~3                             # noqa: E731
    words = lambda n: 2 * up4(3 * 32) + up4(n + 1) + 2 * up4(n) + 2 * up4(n * 10) + 2 * 32 * 32 + up4(n * 32)   # noqa: E731
    assert words(lo) * 4 <= 160 * 1024 < words(lo + 1) * 4


def test_new_entries_refuse_bad_arguments_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    p = ctypes.c_void_p(64)            # never dereferenced: the refusals below come before any launch
    tab = (ctypes.c_void_p * 10)(*[64] * 10)
    null_tab = (ctypes.c_void_p * 10)(*[None] * 10)

    def enc(x=p, vec=p, ei=p, E=8, ptr=p, eptr=p, N=4, B=1, F=9, K=10, hid=32, po=4, layers=1, post=1, dpe=8, dx=8,
            expand=1, table=tab, max_n=4, max_e=8, out=p, pe=None):
        return lib.hscn_signnet_encode(x, vec, ei, E, ptr, eptr, N, B, F, K, hid, po, layers, post, dpe, dx, expand,
                                       table, max_n, max_e, out, pe, None, None)

    assert enc(x=None) == -1 and enc(vec=None) == -1 and enc(ei=None) == -1 and enc(out=None) == -1
    assert enc(ptr=None) == -1 and enc(eptr=None) == -1 and enc(table=None) == -1
    assert enc(N=-1) == -1 and enc(E=-1) == -1 and enc(B=-1) == -1
    assert enc(F=0) == -1 and enc(K=0) == -1 and enc(hid=0) == -1 and enc(po=0) == -1 and enc(dpe=0) == -1
    assert enc(layers=0) == -1 and enc(post=0) == -1 and enc(dx=0) == -1 and enc(max_n=-1) == -1
    assert enc(expand=0, dx=8) == -1                       # without linear_x the leading columns are x: dim_x = F
    assert enc(table=null_tab) == -1                       # a missing weight
    assert enc(hid=65) == -3 and enc(K=65) == -3 and enc(layers=9) == -3 and enc(post=9) == -3
    assert enc(max_n=4000) == -3                           # beyond 160 KB of LDS
    assert enc(B=0) == 0 and enc(N=0, x=None, vec=None, out=None) == 0      # nothing to do: no launch


def test_encoder_engine_attribute_and_named_refusals():
    from graph_hscn.config.config import PEConfig
    from graph_hscn.encoder import SignNetNodeEncoder
    e = SignNetNodeEncoder(PEConfig(9, 16, 8), 9, 16)
    assert e.engine == "layered" and e.last_engine is None
    assert len(e._fused_params()) == 2 * (2 + 1 + 1 + 1)    # Lc = 2 Linear's, the one behind the ReLU, rho, linear_x

    class _B:
        eigvecs_sn = torch.zeros(3, 10)
        x = torch.zeros(3, 9)
    assert "MLP" in SignNetNodeEncoder(PEConfig(9, 16, 8, model="MLP"), 9, 16).fused_reason(_B())
    assert "BatchNorm" in SignNetNodeEncoder(PEConfig(9, 16, 8, use_bn=True), 9, 16).fused_reason(_B())
    assert "gradients" in e.fused_reason(_B())
    e.engine = "fused"
    with pytest.raises(ValueError):
        e(_B_with_vals())


def _B_with_vals():
    class _B:
        eigvecs_sn = torch.zeros(3, 10)
        eigvals_sn = torch.zeros(3, 10, 1)
        x = torch.zeros(3, 9)
    return _B()


@pytest.mark.parametrize("layers,post", [(1, 1), (2, 2), (3, 1), (4, 3)])
def test_the_fold_behind_the_kernel_equals_the_oracle_in_float64(layers, post):
    """csrc/signnet.hip's arrangement, restated in float64: with P = I + A, pre = (P^Lc v) U + sum_l (P^(Lc-1-l) 1) V_l,
    enc = Wb sum_{k < min(K, n)} [relu(c + q_k U) + relu(c - q_k U)] + 2 min(K, n) bb.  Equal to the oracle's 2 K
    passes to float64 rounding."""
    from graph_hscn.config.config import PEConfig
    from graph_hscn.data import Batch
    cfg = PEConfig(3, 12, 5, layers=layers, post_layers=post, eigen_max_freqs=6, phi_hidden_dim=7, phi_out_dim=3)
    torch.manual_seed(layers * 10 + post)
    oe = OS.SignNetNodeEncoder(cfg, 3, 12).double()
    graphs = _ragged(True, "rows")
    b = Batch.from_data_list(graphs)
    with torch.no_grad():
        vec = torch.nan_to_num(b.eigvecs_sn.double(), nan=0.0).unsqueeze(-1)
        want_pe = oe.sign_inv_net(vec, b.edge_index, b.batch)
        fcs = [fc for conv in oe.sign_inv_net.enc.layers for fc in conv.nn.fcs]
        pre, Wb = fcs[:-1], fcs[-1]
        Lc = len(pre)
        assert Lc == max(layers, 2)
        U, V = pre[0].weight[:, 0], [pre[0].bias]
        for fc in pre[1:]:
            U, V = fc.weight @ U, [fc.weight @ v for v in V] + [fc.bias]
        got = []
        for g in graphs:
            n = g.num_nodes
            P = torch.eye(n, dtype=torch.float64)
            P.index_put_((g.edge_index[1], g.edge_index[0]), torch.ones(g.edge_index.size(1), dtype=torch.float64),
                         accumulate=True)
            q = torch.nan_to_num(g.eigvecs_sn.double(), nan=0.0)
            f = torch.ones(n, dtype=torch.float64)
            c = torch.zeros(n, 7, dtype=torch.float64)
            for s in range(Lc):
                c += f[:, None] * V[Lc - 1 - s][None, :]
                q, f = P @ q, P @ f
            cnt = min(6, n)
            acc = sum(torch.relu(c + q[:, k:k + 1] * U) + torch.relu(c - q[:, k:k + 1] * U) for k in range(cnt))
            got.append(oe.sign_inv_net.rho(acc @ Wb.weight.t() + 2 * cnt * Wb.bias))
        got = torch.cat(got, 0)
    assert float((got - want_pe).abs().max()) <= 1e-12 * max(1.0, float(want_pe.abs().max()))
