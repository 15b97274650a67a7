"""The Laplacian-statistics launch (csrc/lap_eig.hip: one workgroup per graph, assembly + parallel-order Jacobi + the
normalised NaN-padded tail) against float64.

The yardstick is never the code under test: ``np.linalg.eigh`` in float64 on ``oracle.signnet.laplacian_dense`` with
its lower triangle mirrored (the matrix ``eigh`` reads; tests/test_posenc_signnet.py does the same).  Eigenvectors are
compared in what is well defined: the eigen-equation, orthogonality, and eigenspace projectors where the float64
spectrum has a gap (asserted, never skipped).

Bounds.  g is the Gershgorin bound of the graph's matrix (backward error scales with the norm; g <= 2 for "sym").
* eigenvalues of the small graphs: the project's atol 2e-5 (test_posenc_signnet.py), times max(1, g/2);
* eigen-equation and orthogonality: 1e-4 * max(1, g/2) (the same file's 1e-4, scaled alike);
* projectors: 1e-3, as there;
* tier-boundary and n = 444 / 500 graphs: max(the bound above, M * the host float32 path's own error on the same
  graph), M = 16.  M's origin: measured on the MI355X with this file's yardstick, the ratio of the device's eigenvalue
  error to the host path's is 3.9 (n = 138 and 139, "sym"), 9.9 (n = 444), 48.9 (n = 500), and 85 / 149 at n = 138 /
  139 under "none".  The smallest power of two above the worst ratio would be 256; M is held at 16, the largest value
  allowed, and the large ratios are a finding that is explained, not widened over: the device errors are 1.5e-7 ..
  5.5e-7 at every one of these graphs, a fraction of float32 roundoff of the matrix norm (matrix and rotations are
  float32, and every round perturbs the off-diagonal entries by their own roundoff) and 36 times under the 2e-5
  floor, while the host path is far better than roundoff of the norm on the few smallest eigenvalues (1.4e-9 ..
  5.9e-8).  Convergence is not the cause: the stopping threshold leaves off^2 / gap < 1e-9.  With M = 16 the floor
  decides at those graphs.  The ratios are printed by ``test_large_graphs`` / ``test_tier_boundary``;
  profiles/r07_posenc_stats.json records them for 10 frequencies against float64 eigh of the host path's own matrix,
  where the host error is as small as 6e-11 and the worst ratio 7.6e3.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import signnet as OS

pytestmark = pytest.mark.gpu

K = 8
M_HOST = 16
LAPS = ("none", "sym", "rw")
VECS = ("L1", "L2", "abs-max")


def _two_way(pairs):
    e = torch.as_tensor(pairs, dtype=torch.long).reshape(-1, 2).t()
    return torch.cat([e, e.flip(0)], 1)


def _path(n):
    return _two_way([(i, i + 1) for i in range(n - 1)])


def _data(n, ei):
    from graph_hscn.data import Data
    return Data(x=torch.zeros(n, 9, dtype=torch.long), edge_index=ei.contiguous(), num_nodes=n)


@functools.lru_cache(maxsize=None)
def _small():
    """name -> graph; one batch mixes them all, so the node and edge offsets are exercised too."""
    from graph_hscn.loader.synthetic import make_dataset
    tri2 = _two_way([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)])                # + node 6, isolated
    dup = torch.cat([_path(5), _two_way([(0, 1)])], 1)                              # edge 0-1 listed twice
    loops = torch.cat([_path(6)[:, :4], torch.tensor([[2, 0], [2, 0]]), _path(6)[:, 4:]], 1)
    t0, t1 = make_dataset("pcqm_contact", 2, seed=5)
    return {
        "n1": _data(1, torch.zeros(2, 0, dtype=torch.long)),
        "n2": _data(2, _path(2)),
        "n3": _data(3, _path(3)),                                                   # odd: an index sits out a round
        "P12": _data(12, _path(12)),
        "C9": _data(9, _two_way([(i, (i + 1) % 9) for i in range(9)])),             # n = K + 1; double eigenvalues
        "S8": _data(8, _two_way([(0, i) for i in range(1, 8)])),                    # n = K; 1 six times under sym
        "tri2": _data(7, tri2),                                                     # n < K; zero three times
        "dup": _data(5, dup),
        "loops": _data(6, loops),
        "tree0": _data(t0.num_nodes, t0.edge_index),
        "tree1": _data(t1.num_nodes, t1.edge_index),
    }


@functools.lru_cache(maxsize=None)
def _f64(ei_key, n, lap, undirected=True):
    """(L float64 with the lower triangle mirrored, eigenvalues, eigenvectors, Gershgorin bound) -- computed once."""
    L = OS.laplacian_dense(ei_key.t, n, None if lap == "none" else lap, undirected).astype(np.float64)
    L = np.tril(L) + np.tril(L, -1).T
    lam, V = np.linalg.eigh(L)
    return L, lam, V, float(np.abs(L).sum(1).max())


class _Key:
    """Hashable handle of an edge_index for the cache."""

    def __init__(self, t):
        self.t = t

    def __hash__(self):
        return id(self.t)

    def __eq__(self, o):
        return self.t is o.t


def _cfg(lap="sym", vec="L2", k=K):
    from graph_hscn.config.config import PEConfig
    return PEConfig(9, 16, 8, eigen_max_freqs=k, eigen_laplacian_norm=lap, eigvec_norm=vec)


def _run(graphs, cfg, undirected=True):
    from graph_hscn.data import Batch
    from graph_hscn.transform import compute_posenc_stats_device
    b = Batch.from_data_list(list(graphs)).to("cuda")
    compute_posenc_stats_device(b, undirected, cfg)
    torch.cuda.synchronize()
    return b


def _unit(V):
    return V / np.linalg.norm(V, axis=0, keepdims=True)


def _check_graph(name, g, vals, vecs, lap, vec, k, eig_bound=None, res_bound=None):
    """Checks 1-3 and 5 of one graph's rows; returns (eigenvalue error, residual, V unit float64, float64 parts)."""
    n = g.num_nodes
    kk = min(k, n)
    L, lam, V64, gb = _f64(_Key(g.edge_index), n, lap)
    scale = max(1.0, gb / 2)
    assert vals.shape == (n, k, 1) and vecs.shape == (n, k)
    # 5: padding exactly [:, n:], eigenvalue rows identical bit for bit, unit columns in the chosen norm
    assert torch.isnan(vals[:, kk:]).all() and torch.isnan(vecs[:, kk:]).all(), name
    assert not torch.isnan(vals[:, :kk]).any() and not torch.isnan(vecs[:, :kk]).any(), name
    assert torch.equal(vals[:, :kk].view(torch.int32), vals[:1, :kk].view(torch.int32).expand(n, kk, 1)), name
    Vn = vecs[:, :kk].numpy().astype(np.float64)
    norms = {"L1": np.abs(Vn).sum(0), "L2": np.sqrt((Vn * Vn).sum(0)), "abs-max": np.abs(Vn).max(0)}[vec]
    assert np.abs(norms - 1).max() < 1e-6, (name, norms)
    # 1: eigenvalues
    got = vals[0, :kk, 0].numpy().astype(np.float64)
    e_dev = float(np.abs(got - np.maximum(lam[:kk], 0)).max())
    bound = 2e-5 * scale if eig_bound is None else eig_bound
    assert e_dev <= bound, (name, lap, e_dev, bound)
    # 2: eigen-equation with the unclamped float64 eigenvalues, 3: orthogonality
    V = _unit(Vn)
    res = float(np.abs(L @ V - V * lam[None, :kk]).max())
    orth = float(np.abs(V.T @ V - np.eye(kk)).max())
    rb = 1e-4 * scale if res_bound is None else res_bound
    assert res < rb, (name, lap, res, rb)
    assert orth < rb, (name, lap, orth, rb)
    return e_dev, res, V, (L, lam, V64, gb)


def _check_projector(name, V, lam, V64, k):
    """4: the span of the first k vectors against float64's, where the spectrum has a gap behind the k-th value."""
    assert lam[k] - lam[k - 1] > 1e-3, (name, k, lam[k] - lam[k - 1])
    P, P64 = V[:, :k] @ V[:, :k].T, V64[:, :k] @ V64[:, :k].T
    assert np.abs(P - P64).max() < 1e-3, (name, k, np.abs(P - P64).max())


def _split(b):
    ptr = b.ptr.tolist()
    vals, vecs = b.eigvals_sn.cpu(), b.eigvecs_sn.cpu()
    return [(vals[ptr[i]:ptr[i + 1]], vecs[ptr[i]:ptr[i + 1]]) for i in range(len(ptr) - 1)]


@pytest.mark.parametrize("vec", VECS)
@pytest.mark.parametrize("lap", LAPS)
def test_small_batch_every_setting(lap, vec):
    graphs = _small()
    b = _run(graphs.values(), _cfg(lap, vec))
    assert int(b.lap_eig_flag.item()) == 0
    parts = {}
    for (name, g), (vals, vecs) in zip(graphs.items(), _split(b)):
        parts[name] = _check_graph(name, g, vals, vecs, lap, vec, K)
    # closed forms: a single node is 0 under "none" and 1 under "sym" / "rw"
    vals = _split(b)[0][0]
    assert float(vals[0, 0, 0]) == (0.0 if lap == "none" else 1.0) and torch.isnan(vals[0, 1:, 0]).all()
    if lap == "none":
        np.testing.assert_allclose(parts["tri2"][3][1][:3], 0, atol=1e-6)             # three components
    if lap == "sym":
        lam = parts["S8"][3][1]
        np.testing.assert_allclose(lam, [0] + [1] * 6 + [2], atol=1e-6)
        np.testing.assert_allclose(parts["tri2"][3][1][:3], [0, 0, 1], atol=1e-6)     # the isolated node: diagonal 1
        for name, k in (("P12", 8), ("C9", 5), ("S8", 1), ("S8", 7), ("tree0", 8), ("tree1", 8)):
            _, _, V, (_, lam, V64, _) = parts[name]
            _check_projector(name, V, lam, V64, k)


def test_one_way_edges_are_symmetrised_when_not_undirected():
    n = 7
    one_way = torch.stack([torch.arange(n - 1), torch.arange(1, n)])
    # pairs listed in both directions, and one listed twice: merged, not summed
    messy = torch.cat([one_way, torch.tensor([[3, 4, 0], [2, 3, 1]])], 1)
    cfg = _cfg("none")
    a = _run([_data(n, messy), _data(2, one_way[:, :1])], cfg, undirected=False)
    b = _run([_data(n, _path(n)), _data(2, _path(2))], cfg, undirected=True)
    assert int(a.lap_eig_flag.item()) == 0
    assert torch.equal(a.eigvals_sn.view(torch.int32), b.eigvals_sn.view(torch.int32))
    assert torch.equal(a.eigvecs_sn.view(torch.int32), b.eigvecs_sn.view(torch.int32))
    _, lam, _, _ = _f64(_Key(messy), n, "none", False)
    np.testing.assert_allclose(a.eigvals_sn[0, :n, 0].cpu().numpy(), np.maximum(lam, 0), atol=2e-5 * 2)


def test_repeatable_and_list_form_equals_batch_form():
    from graph_hscn.transform import compute_posenc_stats_device
    graphs = _small()
    cfg = _cfg()
    a, b = _run(graphs.values(), cfg), _run(graphs.values(), cfg)
    assert int(a.lap_eig_flag.item()) == 0 and int(b.lap_eig_flag.item()) == 0
    assert torch.equal(a.eigvals_sn.view(torch.int32), b.eigvals_sn.view(torch.int32))
    assert torch.equal(a.eigvecs_sn.view(torch.int32), b.eigvecs_sn.view(torch.int32))
    assert a.eigvals_sn.is_cuda and a.eigvals_sn.shape == (a.num_nodes, K, 1) and a.eigvecs_sn.shape == (a.num_nodes, K)
    fresh = [_data(g.num_nodes, g.edge_index) for g in graphs.values()]
    out = compute_posenc_stats_device(fresh, True, cfg, device="cuda")
    assert all(not g.eigvecs_sn.is_cuda and g.eigvals_sn.shape == (g.num_nodes, K, 1) for g in out)
    assert torch.equal(torch.cat([g.eigvals_sn for g in out]).view(torch.int32), a.eigvals_sn.cpu().view(torch.int32))
    assert torch.equal(torch.cat([g.eigvecs_sn for g in out]).view(torch.int32), a.eigvecs_sn.cpu().view(torch.int32))


def test_bad_edges_and_unsupported_sizes_are_reported():
    from graph_hscn.transform import compute_posenc_stats_device
    good, bad = _data(4, _path(4)), _data(3, torch.tensor([[0, 1, 2], [1, 0, 5]]))
    with pytest.raises(RuntimeError, match="graph 1 "):
        compute_posenc_stats_device([good, bad], True, _cfg(), device="cuda")
    with pytest.raises(RuntimeError, match="512"):
        compute_posenc_stats_device([_data(513, _path(513))], True, _cfg(), device="cuda")
    with pytest.raises(RuntimeError, match="64"):
        compute_posenc_stats_device([good], True, _cfg(k=65), device="cuda")


def _host_errors(g, lap, k):
    """The host float32 path (the reference's own arithmetic) against float64 on the same graph."""
    from graph_hscn.transform import compute_posenc_stats
    L, lam, _, _ = _f64(_Key(g.edge_index), g.num_nodes, lap)
    h = compute_posenc_stats(_data(g.num_nodes, g.edge_index), True, _cfg(lap, "L2", k))
    e = float(np.abs(h.eigvals_sn[0, :k, 0].numpy().astype(np.float64) - np.maximum(lam[:k], 0)).max())
    V = _unit(h.eigvecs_sn[:, :k].numpy().astype(np.float64))
    return e, float(np.abs(L @ V - V * lam[None, :k]).max())


def _check_large(graphs, lap, projector_k):
    b = _run(graphs.values(), _cfg(lap))
    assert int(b.lap_eig_flag.item()) == 0
    for (name, g), (vals, vecs) in zip(graphs.items(), _split(b)):
        gb = _f64(_Key(g.edge_index), g.num_nodes, lap)[3]
        e_host, r_host = _host_errors(g, lap, K)
        eb = max(2e-5 * max(1.0, gb / 2), M_HOST * e_host)
        rb = max(1e-4 * max(1.0, gb / 2), M_HOST * r_host)
        e_dev, res, V, (_, lam, V64, _) = _check_graph(name, g, vals, vecs, lap, "L2", K, eb, rb)
        print(f"lap_eig {name} {lap}: e_dev {e_dev:.3e} e_host {e_host:.3e} ratio {e_dev / max(e_host, 1e-30):.2f} "
              f"res_dev {res:.3e} res_host {r_host:.3e} sweeps {b.lap_eig_sweeps.tolist()}")
        if name in projector_k:
            _check_projector(name, V, lam, V64, projector_k[name])
    return b


@functools.lru_cache(maxsize=None)
def _boundary_graphs():
    from graph_hscn import _hip
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    m = _hip.lib().hscn_lap_eig_lds_max_n()
    rng = np.random.default_rng(7)
    a, b = make_graph(rng, SHAPES["peptides_func"], n=m), make_graph(rng, SHAPES["peptides_func"], n=m + 1)
    return {"lds_edge": _data(m, a.edge_index), "global_edge": _data(m + 1, b.edge_index)}


@functools.lru_cache(maxsize=None)
def _large_graphs():
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    rng = np.random.default_rng(11)
    a, b = make_graph(rng, SHAPES["peptides_func"], n=444), make_graph(rng, SHAPES["pascalvoc_sp"], n=500)
    return {"n444": _data(444, a.edge_index), "n500": _data(500, b.edge_index)}


@pytest.mark.parametrize("lap", ["sym", "none"])
def test_tier_boundary(lap):
    """The largest graph the LDS tier takes and the smallest the global tier takes, in one batch (float64 gaps behind
    the 7th eigenvalue under "sym": 5.8e-3 and 8.4e-3)."""
    _check_large(_boundary_graphs(), lap, {"lds_edge": 7, "global_edge": 7} if lap == "sym" else {})


@pytest.mark.parametrize("n", [82, 84])
def test_lds_opt_in_line(n):
    """A launch sized for n = 82 asks for 54 448 bytes of dynamic LDS, which with the kernel's 8 832 bytes of static
    scratch stays within the 64 KB a launch gets unasked; one sized for n = 84 asks for 57 120: over the line with the
    scratch, under it without.  Each launch: a batch of this graph and a smaller one."""
    from graph_hscn.loader.synthetic import SHAPES, make_graph
    rng = np.random.default_rng(n)
    a, b = make_graph(rng, SHAPES["peptides_func"], n=n), make_graph(rng, SHAPES["peptides_func"], n=n - 3)
    _check_large({f"n{n}": _data(n, a.edge_index), f"n{n - 3}": _data(n - 3, b.edge_index)}, "sym", {})


def test_large_graphs():
    """Peptides' largest (444) and PascalVOC-SP's largest (500) graph through the global tier."""
    _check_large(_large_graphs(), "sym", {})


def test_posenc_stage_computes_its_statistics_on_the_device():
    from graph_hscn.config.config import PEConfig
    from graph_hscn.data import Batch, DataLoader
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.train.train import compute_posenc
    from graph_hscn.transform import compute_posenc_stats

    class _DataCfg:
        batch_size = 3

    cfg = PEConfig(9, 16, 6, model="DeepSet", layers=3, post_layers=2, eigen_max_freqs=5, phi_hidden_dim=16, phi_out_dim=4)
    graphs = make_dataset("pcqm_contact", 5, seed=9)
    torch.manual_seed(4)
    _, flat = compute_posenc([DataLoader(graphs, batch_size=3)], _DataCfg, 9, cfg, device="cuda", stats="device")
    enc = compute_posenc.last_encoder
    assert enc.last_engine == "resident" and len(flat) == 2
    oe = OS.SignNetNodeEncoder(cfg, 9, 16)
    oe.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    oe.eval()
    for i, enc_b in enumerate(flat):
        assert int(enc_b.lap_eig_flag.item()) == 0
        host = Batch.from_data_list(graphs[3 * i:3 * i + 3])
        assert enc_b.eigvecs_sn.is_cuda and enc_b.eigvecs_sn.shape == (host.num_nodes, 5)
        with torch.no_grad():
            want, _ = oe(host.x.float(), enc_b.eigvecs_sn.cpu(), host.edge_index, host.batch)
        assert torch.allclose(enc_b.x.cpu(), want, atol=2e-5, rtol=1e-4), float((enc_b.x.cpu() - want).abs().max())
    # the default: pre-computed statistics go through unchanged
    pre = make_dataset("pcqm_contact", 5, seed=9)
    for g in pre:
        compute_posenc_stats(g, True, cfg)
    _, flat0 = compute_posenc([DataLoader(pre, batch_size=3)], _DataCfg, 9, cfg, device="cuda")
    oe.load_state_dict({k: v.cpu() for k, v in compute_posenc.last_encoder.state_dict().items()})
    for i, enc_b in enumerate(flat0):
        host = Batch.from_data_list(pre[3 * i:3 * i + 3])
        assert not hasattr(enc_b, "lap_eig_flag")
        assert torch.equal(enc_b.eigvecs_sn.cpu().view(torch.int32), host.eigvecs_sn.view(torch.int32))
        with torch.no_grad():
            want, _ = oe(host.x.float(), host.eigvecs_sn, host.edge_index, host.batch)
        assert torch.allclose(enc_b.x.cpu(), want, atol=2e-5, rtol=1e-4)
