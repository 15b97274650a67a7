"""Random-walk structural encoding on the device (include/hscn.h: hscn_rwse_stats, csrc/rwse.hip) against a float64
referee written here, independent of the package's host path: dense A by index_put_(accumulate=True) in float64,
P = dinv[:, None] * A, M = P @ M K times, diagonal(M) each time.

Bound (helpers.f64_close, c = 3): mag = |ref| element-wise, n = k * (dmax + 2) for column k, dmax the largest
out-degree of the batch.  Every term is non-negative; one step is a sum of at most dmax terms plus the reciprocal and
the multiply, a relative error of at most (dmax + 1) 2^-24; a non-negative linear map passes relative input errors on
unamplified, so k steps give k (dmax + 1), and the +1 covers second order.  An entry whose reference is exactly 0 (no
closed walk of that length) must be exactly 0: f64_close's ``tiny`` makes that an equality test.

Teeth, both asserted in float64 on the CPU before the device is touched, then used as ``dropped`` in check_f64:
(a) the reference with one listed edge left out; (b) in-degree instead of out-degree normalisation on a list with
one-directional edges."""
import pytest
import torch

from graph_hscn.loader.synthetic import make_dataset
from tests.helpers import DEV, F64_C, U32, check_f64, close, f64_close

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- #
# the referee
# --------------------------------------------------------------------------- #
def _ref_graph(ei, n, K, indeg=False):
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[0], ei[1]), torch.ones(ei.size(1), dtype=torch.float64), accumulate=True)
    deg = A.sum(0) if indeg else A.sum(1)
    dinv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    P = dinv[:, None] * A
    M = torch.eye(n, dtype=torch.float64)
    cols = []
    for _ in range(K):
        M = P @ M
        cols.append(torch.diagonal(M).clone())
    return torch.stack(cols, 1)


def _ref(graphs, K, drop=None, indeg=False, full=None):
    """[N, K] float64 over the list; ``drop`` = (graph, edge position) leaves that listed edge out (``full``: the
    reference without ``drop``, whose rows the other graphs keep)."""
    rows, o = [], 0
    for b, g in enumerate(graphs):
        ei, n = g.edge_index, int(g.num_nodes)
        if drop is not None and drop[0] == b:
            keep = torch.ones(ei.size(1), dtype=torch.bool)
            keep[drop[1]] = False
            rows.append(_ref_graph(ei[:, keep], n, K, indeg))
        elif drop is not None and full is not None:
            rows.append(full[o:o + n])
        else:
            rows.append(_ref_graph(ei, n, K, indeg))
        o += n
    return torch.cat(rows, 0)


def _dmax(graphs):
    return max(int(torch.bincount(g.edge_index[0], minlength=1).max()) if g.edge_index.numel() else 0 for g in graphs)


def _steps(K, dmax):
    return (torch.arange(1, K + 1, dtype=torch.float64) * (dmax + 2)).unsqueeze(0)


def _outside(ref, other, n):
    """Whether ``other`` lies outside the bound around ``ref`` somewhere (the float64 form of the teeth)."""
    return bool(((other - ref).abs() > F64_C * n * U32 * ref.abs() + 1e-30).any())


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def _edge_graph(n, seed):
    """A ring plus three seeded chords (both directions), a self loop on node 1, the edge 0 -> 1 listed twice and the
    one-directional edge 0 -> n - 1.  From six nodes on the ring runs over nodes 0 .. n - 3, node n - 2 is isolated and
    node n - 1 only receives (a row of P that is all zero while mass flows into it).  Below that every node is on the
    ring; n = 1 is a lone self loop."""
    from graph_hscn.data import Data
    if n == 1:
        edges = [(0, 0)]
    else:
        m = n - 2 if n >= 6 else n
        edges = []
        for i in range(m if m > 2 else 1):
            edges += [(i, (i + 1) % m), ((i + 1) % m, i)]
        g = torch.Generator().manual_seed(seed)
        if m >= 6:
            for _ in range(3):
                a, b = torch.randperm(m, generator=g)[:2].tolist()
                edges += [(a, b), (b, a)]
        edges += [(1, 1), (0, 1), (0, n - 1)]
    ei = torch.tensor(edges, dtype=torch.int64).t().contiguous()
    return Data(x=torch.zeros(n, 1), edge_index=ei, y=torch.zeros(1, 1), num_nodes=n)


def _cfg(K):
    from graph_hscn.config.config import RWSEConfig
    return RWSEConfig(9, 16, 8, ksteps=K)


def _tile():
    from graph_hscn import _hip
    return int(_hip.lib().hscn_rwse_tile())


def _device_batch(graphs):
    from graph_hscn.data import Batch
    return Batch.from_data_list(graphs).to(DEV)


def _device_rwse(graphs, K, is_undirected=True):
    from graph_hscn.transform import compute_rwse_stats_device
    b = compute_rwse_stats_device(_device_batch(graphs), is_undirected, _cfg(K))
    assert b.rwse.dtype == torch.float32 and tuple(b.rwse.shape) == (int(b.num_nodes), K)
    assert b.rwse_flag.dtype == torch.int32 and tuple(b.rwse_flag.shape) == (1,)
    return b.rwse.cpu(), int(b.rwse_flag.item())


_CACHE = {}


def _edge_case(which):
    """(graphs, float64 reference at the largest K used, the two teeth, dmax), computed once and never modified."""
    if which not in _CACHE:
        T = _tile()
        if which == "small":
            graphs, K = [_edge_graph(n, 10 + n) for n in (1, 2, T - 1, T, T + 1, 2 * T + 1)], 64
        else:
            graphs, K = [_edge_graph(512, 5)], 20
        last = len(graphs) - 1
        pos = [tuple(e) for e in graphs[last].edge_index.t().tolist()].index((1, 0))     # an out-edge of the loop's node
        ref = _ref(graphs, K)
        _CACHE[which] = (graphs, ref, _ref(graphs, K, drop=(last, pos), full=ref), _ref(graphs, K, indeg=True),
                         _dmax(graphs))
    return _CACHE[which]


# --------------------------------------------------------------------------- #
# tile edges
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("which,K", [("small", 1), ("small", 20), ("small", 64), ("large", 1), ("large", 20)])
def test_tile_edges_against_float64(which, K):
    graphs, ref, no_edge, by_indeg, dmax = _edge_case(which)
    ref, no_edge, by_indeg = ref[:, :K], no_edge[:, :K], by_indeg[:, :K]        # column k does not depend on K
    n = _steps(K, dmax)
    assert _outside(ref, no_edge, n) and _outside(ref, by_indeg, n)
    got, flag = _device_rwse(graphs, K)
    assert flag == 0
    check_f64(got, ref, ref.abs(), n, no_edge, what=f"{which} K={K} [edge dropped]")
    check_f64(got, ref, ref.abs(), n, by_indeg, what=f"{which} K={K} [in-degree]")
    assert bool((got[ref == 0] == 0).all())
    # the isolated node and the node without out-edges (the last two nodes of every graph of six nodes or more)
    o = 0
    for g in graphs:
        if g.num_nodes >= 6:
            assert bool((got[o + g.num_nodes - 2:o + g.num_nodes] == 0).all())
        o += g.num_nodes


# --------------------------------------------------------------------------- #
# shaped batches
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name,count", [("peptides_func", 8), ("pcqm_contact", 16), ("pascalvoc_sp", 2)])
def test_shaped_batches_against_float64(name, count):
    from graph_hscn.transform import compute_rwse_stats_device
    K = 20
    graphs = make_dataset(name, count, seed=3)
    ref = _ref(graphs, K)
    no_edge = _ref(graphs, K, drop=(0, 0), full=ref)
    n = _steps(K, _dmax(graphs))
    assert _outside(ref, no_edge, n)
    got, flag = _device_rwse(graphs, K)
    assert flag == 0
    check_f64(got, ref, ref.abs(), n, no_edge, what=f"{name} [edge dropped]")
    # the list form: per-graph CPU tensors, the batch form's rows
    out = compute_rwse_stats_device(graphs, True, _cfg(K))
    assert out[0] is graphs[0]
    o = 0
    for g in out:
        assert not g.rwse.is_cuda and torch.equal(g.rwse, got[o:o + g.num_nodes])
        o += g.num_nodes
    for g in graphs:
        del g._d["rwse"]


def test_directed_list_is_symmetrised_first():
    """``is_undirected=False`` on a list with half of its reverse edges removed equals ``is_undirected=True`` on the
    full list.  The full list is taken in the order ``_undirected`` produces (sorted, duplicates merged), so that both
    calls walk the same CSR rows in the same order and the comparison is one of bits."""
    from graph_hscn.data import Data
    from graph_hscn.transform import compute_rwse_stats_device
    from graph_hscn.transform.posenc import _undirected
    full, half = [], []
    for g in make_dataset("pcqm_contact", 6, seed=4):
        ei = _undirected(g.edge_index)
        back = (ei[0] > ei[1]).nonzero().flatten()
        keep = torch.ones(ei.size(1), dtype=torch.bool)
        keep[back[::2]] = False
        assert 0 < int(keep.sum()) < ei.size(1)
        full.append(Data(x=g.x, edge_index=ei, y=g.y, num_nodes=g.num_nodes))
        half.append(Data(x=g.x, edge_index=ei[:, keep].contiguous(), y=g.y, num_nodes=g.num_nodes))
    a = compute_rwse_stats_device(full, True, _cfg(20))
    b = compute_rwse_stats_device(half, False, _cfg(20))
    for ga, gb in zip(a, b):
        assert torch.equal(ga.rwse, gb.rwse)
    # and as given, the halved list is another walk
    c, _ = _device_rwse(half, 20, True)
    assert not torch.equal(c, torch.cat([g.rwse for g in a], 0))


# --------------------------------------------------------------------------- #
# determinism and capture
# --------------------------------------------------------------------------- #
def _raw(batch, K, max_n=None, col=None):
    """One hscn_rwse_stats launch over the batch's source-keyed CSR: (launch, rw, flag)."""
    from graph_hscn import _hip
    from graph_hscn.structure import build_csr
    N, B = int(batch.num_nodes), int(batch.num_graphs)
    csr = build_csr(batch.edge_index[0], batch.edge_index[1], N, N)
    col = csr.col if col is None else col(csr)
    rw = torch.full((N, K), -1.0, dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    max_n = int(batch.max_nodes) if max_n is None else max_n

    def launch():
        _hip.call("hscn_rwse_stats", _hip.ptr(csr.rowptr), _hip.ptr(col), _hip.ptr(batch.ptr32), N, B, max_n, K,
                  _hip.ptr(rw), _hip.ptr(flag), _hip.stream())
    return launch, rw, flag


def test_two_launches_give_equal_bits_and_a_captured_launch_replays():
    graphs = make_dataset("peptides_func", 8, seed=3)
    batch = _device_batch(graphs)
    launch, rw, flag = _raw(batch, 20)                       # the CSR is built here, before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
        first = rw.clone()
        launch()
        second = rw.clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and int(flag.item()) == 0
    assert torch.equal(first.cpu(), _device_rwse(graphs, 20)[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        rw.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rw, first)


# --------------------------------------------------------------------------- #
# flags
# --------------------------------------------------------------------------- #
def test_an_entry_outside_its_graph_sets_bit_1():
    graphs, ref, _, _, dmax = _edge_case("small")
    batch = _device_batch(graphs)
    N = int(batch.num_nodes)

    def col(csr):
        c = csr.col.clone()
        c[0] = N - 1                      # graph 0's only entry now names a node of the last graph: inside [0, N)
        return c
    launch, rw, flag = _raw(batch, 4, col=col)
    launch()
    torch.cuda.synchronize()
    assert int(flag.item()) == 2
    got = rw.cpu()
    assert bool((got[0] == 0).all())                           # the entry added nothing to its sum
    assert f64_close(got[1:], ref[1:, :4], ref[1:, :4].abs(), _steps(4, dmax), what="the other graphs")


def test_a_graph_beyond_max_n_sets_bit_2_and_gets_nan_rows():
    graphs, ref, _, _, dmax = _edge_case("small")
    T = _tile()
    batch = _device_batch(graphs)
    big = int(batch.ptr[-2])                                   # the last graph (2 T + 1 nodes) starts here
    launch, rw, flag = _raw(batch, 20, max_n=T + 1)
    launch()
    torch.cuda.synchronize()
    assert int(flag.item()) == 4
    got = rw.cpu()
    assert bool(torch.isnan(got[big:]).all()) and not bool(torch.isnan(got[:big]).any())
    assert f64_close(got[:big], ref[:big, :20], ref[:big, :20].abs(), _steps(20, dmax), what="the other graphs")


def test_the_list_form_names_the_graph():
    from graph_hscn.data import Data
    from graph_hscn.transform import compute_rwse_stats_device
    graphs = make_dataset("pcqm_contact", 3, seed=5)

    def broken(b, node):
        out = []
        for i, g in enumerate(graphs):
            ei = g.edge_index.clone()
            if i == b:
                ei[1, 0] = node
            out.append(Data(x=g.x, edge_index=ei, y=g.y, num_nodes=g.num_nodes))
        return out
    # an end in the next graph's node range (inside [0, N)), and one beyond the whole batch
    with pytest.raises(RuntimeError, match=r"compute_rwse_stats_device: graph 1 has an edge with an end outside"):
        compute_rwse_stats_device(broken(1, graphs[1].num_nodes), True, _cfg(4))
    with pytest.raises(RuntimeError, match=r"compute_rwse_stats_device: graph 2 has an edge with an end outside"):
        compute_rwse_stats_device(broken(2, graphs[2].num_nodes), True, _cfg(4))


# --------------------------------------------------------------------------- #
# the encoder
# --------------------------------------------------------------------------- #
def _torch_encoder(enc, x, rw):
    """The encoder's forward with plain torch on the CPU from copies of its weights (training-mode BatchNorm)."""
    import torch.nn.functional as F
    p = {n: v.detach().cpu().clone().requires_grad_() for n, v in enc.named_parameters()}
    pe = rw
    if enc.raw_norm is not None:
        pe = F.batch_norm(pe, None, None, p["raw_norm.weight"], p["raw_norm.bias"], training=True, eps=enc.raw_norm.eps)
    for i in range(len(enc.pe_encoder)):
        pe = F.linear(pe, p[f"pe_encoder.{i}.weight"], p[f"pe_encoder.{i}.bias"])
        if enc.model_type == "mlp":
            pe = torch.relu(pe)
    h = F.linear(x, p["linear_x.weight"], p["linear_x.bias"])
    return torch.cat((h, pe), 1), pe, p


@pytest.mark.parametrize("raw_norm", ["none", "batchnorm"])
@pytest.mark.parametrize("model,layers", [("linear", 1), ("mlp", 3)])
def test_encoder_against_plain_torch(model, layers, raw_norm):
    from graph_hscn.config.config import RWSEConfig
    from graph_hscn.encoder import RWSENodeEncoder
    from graph_hscn.transform import compute_rwse_stats_device
    cfg = RWSEConfig(9, 16, 8, ksteps=20, model=model, layers=layers, raw_norm=raw_norm, pass_as_var=True)
    graphs = make_dataset("peptides_func", 8, seed=3)
    batch = _device_batch(graphs)
    batch.x = batch.x.float()
    compute_rwse_stats_device(batch, True, cfg)
    x_cpu, rw_cpu = batch.x.cpu(), batch.rwse.cpu()
    torch.manual_seed(7)
    enc = RWSENodeEncoder(cfg, 9, 16).to(DEV)
    want, want_pe, p = _torch_encoder(enc, x_cpu, rw_cpu)
    out = enc(batch)
    assert out is batch and tuple(batch.x.shape) == (x_cpu.size(0), 16)
    assert close(batch.x, want) and close(batch.pe_rwse, want_pe)
    gy = torch.randn(want.shape, generator=torch.Generator().manual_seed(8))
    want.backward(gy)
    batch.x.backward(gy.to(DEV))
    for name, v in enc.named_parameters():
        assert v.grad is not None, name
        assert close(v.grad, p[name].grad, atol=1e-4, rtol=1e-4), name


# --------------------------------------------------------------------------- #
# the stage
# --------------------------------------------------------------------------- #
def test_compute_posenc_with_an_rwse_config_feeds_stage_a():
    import math

    from graph_hscn.config.config import DataConfig, RWSEConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.encoder import RWSENodeEncoder
    from graph_hscn.model.hscn import SCN
    from graph_hscn.nn.pool import gcn_norm
    from graph_hscn.train import compute_posenc, get_each_data_from_batch
    graphs = make_dataset("peptides_func", 10, seed=6)
    loaders = [DataLoader(graphs[:6], batch_size=4, shuffle=True), DataLoader(graphs[6:], batch_size=4)]
    torch.manual_seed(2)
    new_loaders, flat = compute_posenc(loaders, DataConfig("peptides_func", pe=True, batch_size=4), 9,
                                       RWSEConfig(9, 16, 8), device="cuda")
    assert isinstance(compute_posenc.last_encoder, RWSENodeEncoder)
    assert [len(l) for l in new_loaders] == [2, 1] and len(flat) == 3
    assert new_loaders[0].shuffle and not new_loaders[1].shuffle
    encoded = get_each_data_from_batch(flat)
    assert len(encoded) == 10
    assert all(tuple(g.x.shape) == (g.num_nodes, 16) and tuple(g.rwse.shape) == (g.num_nodes, 20) for g in encoded)
    assert all(int(b.rwse_flag.item()) == 0 for b in flat)
    assert sorted(g.num_nodes for g in encoded) == sorted(g.num_nodes for g in graphs)
    # one stage-A step on an encoded graph
    g0 = encoded[0].to(DEV)
    scn = SCN([16], "elu", 16, 8).to(DEV)
    ei, ew = gcn_norm(g0.edge_index, None, g0.num_nodes, add_self_loops=True)
    _, mc, oo, _ = scn(g0.x.float(), ei, ew)
    loss = mc + oo
    loss.backward()
    assert math.isfinite(float(loss.detach()))
