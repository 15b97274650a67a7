"""The one-launch SignNet encoder (csrc/signnet.hip, include/hscn.h: hscn_signnet_encode) against oracle/signnet.py
evaluated in float64 on the same float32 inputs and weights, its envelope and fallbacks, and the positional-encoding
stage built on it (train.compute_posenc) up to a few resident stage-C epochs.

The bound (helpers.f64_close: |got - ref| <= F64_C n 2^-24 mag, F64_C unchanged).  The encoding is a chain of sums of
products; the kernel evaluates the linear part in front of the one ReLU in another association than the layered path
(W (w0 s) as (W w0) s, the DeepSet sum in front of the last Linear), so the bound is the one that holds for ANY
association: first-order, the rounding errors of the stages add, each at most (length of the stage's sum) x u x (the
chain evaluated on absolute values, ReLU being 1-Lipschitz with relu(|.|) = |.|).

  mag: the oracle's modules with |W|, |b| on |eigvecs| -- every intermediate is then non-negative, so ReLU is the
       identity and the two signs give the same value: mag_pe = rho_abs(sum_{k < min(K, n)} 2 phi_abs(|v_k|)), and
       mag_x = |x| |Wx|^T + |bx| for linear_x's columns.
  n:   Lc = max(layers, 2) neighbour sums of 1 + (largest in-degree) terms each; Linear(1, Hd): 2; the Lc - 1
       Linear(Hd, Hd) in front of the ReLU: Hd + 1 each; ReLU: 4; Linear(Hd, Od): Hd + 1; the sum over 2 K (frequency,
       sign) terms: 2 K; rho: fin + 1 per Linear and 4 per ReLU; 4 for the products the fold adds ((P^j 1) V, q U,
       2 cnt bb).  linear_x: F + 1.

Teeth (helpers.check_f64): the same bound must REJECT the float64 reference with frequency 0 left out of the masked
sum, and the one with one edge left out of one row."""
import copy

import pytest
import torch

from tests.helpers import check_f64, f64_close
from oracle import signnet as OS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cfg(layers=1, post=1, K=10, hid=32, po=4, dim_in=9, dim_emb=16, dim_pe=8, **kw):
    from graph_hscn.config.config import PEConfig
    return PEConfig(dim_in, dim_emb, dim_pe, layers=layers, post_layers=post, eigen_max_freqs=K, phi_hidden_dim=hid,
                    phi_out_dim=po, **kw)


def _pair(cfg, seed, F=9):
    """(oracle in float32, product encoder on the device) holding the same weights."""
    from graph_hscn.encoder import SignNetNodeEncoder
    torch.manual_seed(seed)
    oe = OS.SignNetNodeEncoder(cfg, F, cfg.dim_emb)
    pe = SignNetNodeEncoder(cfg, F, cfg.dim_emb).to(DEV)
    pe.load_state_dict(oe.state_dict())
    return oe, pe


def _graph(n, ei, K, g, F=9):
    from graph_hscn.data import Data
    vec = torch.randn(n, K, generator=g)
    vec[:, min(n, K):] = float("nan")                       # the padding compute_posenc_stats leaves
    return Data(x=torch.randn(n, F, generator=g), edge_index=ei, y=torch.randn(1, 10, generator=g), num_nodes=n,
                eigvecs_sn=vec, eigvals_sn=torch.zeros(n, K, 1))


def _sym(n, e, g):
    a = torch.randint(0, n, (2, e), generator=g)
    return torch.cat([a, a.flip(0)], 1)


def _ragged_batch(K, seed=0):
    """Symmetric graphs of 6, 9 and 14 nodes, a 1-node graph, a 4-node graph without edges, and a 7-node graph with
    repeated, one-way and loop edges."""
    from graph_hscn.data import Batch
    g = torch.Generator().manual_seed(seed)
    odd = torch.tensor([[0, 0, 0, 1, 2, 3, 3, 5, 6], [1, 1, 1, 2, 3, 3, 4, 6, 6]])
    graphs = [_graph(6, _sym(6, 8, g), K, g), _graph(1, torch.zeros(2, 0, dtype=torch.long), K, g),
              _graph(9, _sym(9, 14, g), K, g), _graph(4, torch.zeros(2, 0, dtype=torch.long), K, g),
              _graph(7, odd, K, g), _graph(14, _sym(14, 30, g), K, g)]
    return Batch.from_data_list(graphs)


def _pe64(net, vec, ei, batch_index, drop_freq=None, absolute=False):
    """oracle MaskedGINDeepSigns.forward in float64; ``drop_freq``: that frequency left out of the masked sum;
    ``absolute``: the magnitude chain (the module holds |W|, |b|; both signs give phi(|v|))."""
    x = torch.nan_to_num(vec.double(), nan=0.0).unsqueeze(-1)
    N, K = x.shape[0], x.shape[1]
    x = x.transpose(0, 1)
    x = 2 * net.enc(x.abs(), ei) if absolute else net.enc(x, ei) + net.enc(-x, ei)
    x = x.transpose(0, 1).clone()
    per_node = torch.bincount(batch_index)[batch_index]
    mask = torch.arange(K).unsqueeze(0).expand(N, K) < per_node.unsqueeze(1)
    if drop_freq is not None:
        mask = mask & (torch.arange(K).unsqueeze(0) != drop_freq)
    x[~mask] = 0
    return net.rho(x.sum(dim=1))


def _reference(oe, cfg, b):
    """(ref_x, ref_pe, mag_x, mag_pe, n_x, n_pe, dropped-frequency pe, dropped-edge pe) in float64."""
    o64 = copy.deepcopy(oe).double()
    oabs = copy.deepcopy(o64)
    with torch.no_grad():
        for p in oabs.parameters():
            p.abs_()
        net, ei, bi = o64.sign_inv_net, b.edge_index, b.batch
        ref_pe = _pe64(net, b.eigvecs_sn, ei, bi)
        mag_pe = _pe64(oabs.sign_inv_net, b.eigvecs_sn, ei, bi, absolute=True)
        drop_f = _pe64(net, b.eigvecs_sn, ei, bi, drop_freq=0)
        drop_e = _pe64(net, b.eigvecs_sn, ei[:, 1:], bi) if ei.size(1) else None
        ref_x = o64.linear_x(b.x.double())
        mag_x = oabs.linear_x(b.x.double().abs())
    Lc, Hd, Od, K = max(cfg.layers, 2), cfg.phi_hidden_dim, cfg.phi_out_dim, cfg.eigen_max_freqs
    dmax = int(torch.bincount(ei[1], minlength=1).max()) if ei.size(1) else 0
    n_pe = Lc * (1 + dmax) + 2 + (Lc - 1) * (Hd + 1) + 4 + (Hd + 1) + 2 * K + 4
    R = cfg.post_layers
    for r in range(R):
        n_pe += (Od if r == 0 else Hd) + 1 + (4 if r < R - 1 else 0)
    return ref_x, ref_pe, mag_x, mag_pe, b.x.size(1) + 1, n_pe, drop_f, drop_e


def _run(pe, b, engine="resident"):
    d = b.to(DEV)
    d.x = d.x.float()
    pe.engine = engine
    with torch.no_grad():
        out = pe(d)
    torch.cuda.synchronize()
    return out


def _check(oe, pe, cfg, b, what):
    out = _run(pe, b)
    assert pe.last_engine == "resident" and int(pe._resident_flag) == 0
    dx = cfg.dim_emb - cfg.dim_pe
    assert out.x.shape == (b.num_nodes, cfg.dim_emb) and out.x.dtype == torch.float32
    ref_x, ref_pe, mag_x, mag_pe, n_x, n_pe, drop_f, drop_e = _reference(oe, cfg, b)
    got_x, got_pe = out.x[:, :dx].cpu(), out.x[:, dx:].cpu()
    print(what, "pe distance", float((got_pe.double() - ref_pe).abs().max()), "largest limit",
          float((3.0 * n_pe * 2.0 ** -24 * mag_pe).max()), "n", n_pe)
    assert f64_close(got_x, ref_x, mag_x, n_x, what=what + " linear_x")
    check_f64(got_pe, ref_pe, mag_pe, n_pe, drop_f, what=what + " pe (frequency 0 dropped)")
    if drop_e is not None:
        check_f64(got_pe, ref_pe, mag_pe, n_pe, drop_e, what=what + " pe (edge 0 dropped)")
    return out


@pytest.mark.parametrize("K", [1, 3, 4, 6, 10])           # 4 = the smallest multi-node graph; 1 = the 1-node graph
@pytest.mark.parametrize("post", [1, 2])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_fused_encoder_within_the_float64_bound(layers, post, K):
    cfg = _cfg(layers, post, K, hid=16 if K < 10 else 32)
    oe, pe = _pair(cfg, seed=layers * 100 + post * 10 + K)
    _check(oe, pe, cfg, _ragged_batch(K, seed=K), f"layers={layers} post={post} K={K}")


def test_pass_as_var_and_sign_flip():
    cfg = _cfg(2, 2, 6, pass_as_var=True)
    oe, pe = _pair(cfg, seed=5)
    b = _ragged_batch(6, seed=3)
    out = _check(oe, pe, cfg, b, "pass_as_var")
    assert torch.equal(out.pe_SignNet, out.x[:, 8:])
    b2 = _ragged_batch(6, seed=3)
    b2.eigvecs_sn = -b2.eigvecs_sn
    out2 = _run(pe, b2)
    # -v negates every gathered sum exactly and swaps the two ReLU terms of a commutative addition
    lim = 4 * 2.0 ** -23 * float(out.x.abs().max())
    assert float((out2.x - out.x).abs().max()) <= lim


@pytest.mark.parametrize("n,e", [(444, 1332), (500, 1500)])      # Peptides' largest graph (2 664 edges), PascalVOC-SP's
def test_largest_shapes(n, e):
    from graph_hscn.data import Batch
    cfg = _cfg()                                                  # the defaults: hidden 32, K = 10, one layer each
    oe, pe = _pair(cfg, seed=n)
    g = torch.Generator().manual_seed(n)
    ring = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    rest = torch.randint(0, n, (2, e - n), generator=g)
    ei = torch.cat([ring, rest], 1)
    ei = torch.cat([ei, ei.flip(0)], 1)
    assert ei.size(1) == 2 * e
    b = Batch.from_data_list([_graph(n, ei, 10, g), _graph(12, _sym(12, 20, g), 10, g)])
    _check(oe, pe, cfg, b, f"n={n}")


def _outside(case):
    from graph_hscn.data import Batch
    g = torch.Generator().manual_seed(11)
    cfg = _cfg(2, 1, 6, use_bn=(case == "use_bn"))
    b = _ragged_batch(6, seed=2)
    if case == "oversize":
        b = Batch.from_data_list([_graph(6000, _sym(6000, 3000, g), 6, g), _graph(5, _sym(5, 6, g), 6, g)])
    return cfg, b


@pytest.mark.parametrize("case,word", [("use_bn", "BatchNorm"), ("grad", "gradients"), ("oversize", "envelope"),
                                       ("float64", "float32")])
def test_outside_the_envelope_auto_is_layered_and_resident_raises(case, word):
    import contextlib
    cfg, b = _outside(case)
    _, pe = _pair(cfg, seed=9)
    ctx = contextlib.nullcontext() if case == "grad" else torch.no_grad()

    def run(engine):
        d = b.to(DEV)
        d.x = d.x.double() if case == "float64" else d.x.float()
        pe.engine = engine
        with ctx:
            return pe(d).x.detach()

    want = run("layered")
    assert pe.last_engine == "layered"
    pe.last_engine = None
    got = run("auto")
    assert pe.last_engine == "layered" and torch.equal(got, want)
    with pytest.raises(RuntimeError, match=word):
        run("resident")


def test_a_bad_edge_raises_the_flag_and_faults_nothing():
    cfg = _cfg(2, 1, 6)
    _, pe = _pair(cfg, seed=2)
    good = _run(pe, _ragged_batch(6, seed=4)).x.clone()
    b = _ragged_batch(6, seed=4)
    assert int(b.ptr[2]) == 7 and int(b.eptr32[1]) == 16     # graph 0: nodes 0..5, edges 0..15
    b.edge_index[0, 3] = 9                                    # an edge of graph 0 whose source lies in graph 2
    out = _run(pe, b)
    assert pe.last_engine == "resident" and int(pe._resident_flag) & 1
    assert bool(torch.isfinite(out.x).all())
    assert torch.equal(out.x[6:], good[6:])                   # the other graphs are untouched


def _peptides_loaders(cfg, count=40, bs=8):
    from graph_hscn.data import DataLoader
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.transform import compute_posenc_stats
    graphs = make_dataset("peptides_func", count, seed=6)
    for g in graphs:
        compute_posenc_stats(g, True, cfg)
    a, c = count * 6 // 10, count * 8 // 10
    return graphs, [DataLoader(graphs[:a], batch_size=bs, shuffle=True), DataLoader(graphs[a:c], batch_size=bs),
                    DataLoader(graphs[c:], batch_size=bs)]


def test_compute_posenc_on_three_loaders():
    from graph_hscn.config.config import DataConfig
    from graph_hscn.encoder import SignNetNodeEncoder
    from graph_hscn.train import compute_posenc, get_each_data_from_batch
    cfg = _cfg()
    graphs, loaders = _peptides_loaders(cfg)
    torch.manual_seed(3)
    new_loaders, flat = compute_posenc(loaders, DataConfig("peptides_func", pe=True, batch_size=8), 9, cfg, None)
    enc = compute_posenc.last_encoder
    assert enc.engine == "auto" and enc.last_engine == "resident"
    assert [len(l) for l in new_loaders] == [3, 1, 1] and len(flat) == 5
    assert new_loaders[0].shuffle and not new_loaders[1].shuffle and not new_loaders[2].shuffle
    assert all(bt.x.shape[1] == 16 and bt.x.is_cuda for bt in flat)
    each = get_each_data_from_batch(flat)
    assert len(each) == 40 and all(g.x.shape == (g.num_nodes, 16) for g in each)
    # loaders 1 and 2 keep the order of the input: graph by graph the edge lists and targets of the source
    for lo, src in ((1, graphs[24:32]), (2, graphs[32:])):
        assert [g.num_nodes for g in new_loaders[lo].dataset] == [g.num_nodes for g in src]
        assert all(torch.equal(g.edge_index.cpu(), s.edge_index) and torch.equal(g.y.cpu(), s.y)
                   for g, s in zip(new_loaders[lo].dataset, src))
        bt = next(iter(new_loaders[lo]))
        assert bt.num_graphs == 8 and bt.x.shape[1] == 16
    # against the layered encoder holding the same weights: both are float32 evaluations within the bound of the
    # float64 value, so within twice the bound of each other
    lay = SignNetNodeEncoder(cfg, 9, 16).to(DEV)
    lay.load_state_dict(enc.state_dict())
    oe = OS.SignNetNodeEncoder(cfg, 9, 16)
    oe.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    from graph_hscn.data import Batch
    for lo, src in ((1, graphs[24:32]), (2, graphs[32:])):
        b = Batch.from_data_list(src)
        got = torch.cat([g.x for g in new_loaders[lo].dataset], 0).cpu()
        with torch.no_grad():
            d = b.to(DEV)
            d.x = d.x.float()
            want = lay(d).x.cpu()
        assert lay.last_engine == "layered"
        b.x = b.x.float()
        ref_x, ref_pe, mag_x, mag_pe, n_x, n_pe, _, _ = _reference(oe, cfg, b)
        assert f64_close(got[:, 8:], ref_pe, mag_pe, n_pe, what="compute_posenc pe vs float64")
        assert f64_close(got[:, :8], ref_x, mag_x, n_x, what="compute_posenc linear_x vs float64")
        assert f64_close(got[:, 8:], want[:, 8:], mag_pe, 2 * n_pe, what="fused vs layered pe")
        assert f64_close(got[:, :8], want[:, :8], mag_x, 2 * n_x, what="fused vs layered linear_x")


def test_pe_then_stage_a_b_c_keeps_the_one_launch_engines():
    import numpy as np
    from graph_hscn.config.config import ACT_DICT, DataConfig, HSCNConfig, OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.loader.hetero_data import generate_hetero_data
    from graph_hscn.model.hscn import HSCN, SCN
    from graph_hscn.train import compute_posenc, get_each_data_from_batch
    from graph_hscn.train.train_clustering import train_clustering
    from graph_hscn.train.train_resident import fit_resident
    cfg = _cfg()                                              # dim_emb = 16
    _, loaders = _peptides_loaders(cfg)
    loaders[0].shuffle = False
    dc = DataConfig("peptides_func", pe=True, batch_size=8)
    torch.manual_seed(1)
    _, flat = compute_posenc(loaders, dc, 9, cfg, None)
    assert compute_posenc.last_encoder.last_engine == "resident"
    dataset = [g.to("cpu") for g in get_each_data_from_batch(flat)]
    assert len(dataset) == 40 and all(g.x.shape[1] == 16 for g in dataset)
    mc = HSCNConfig("relu", num_clusters=8, cluster_epochs=2)
    scn = SCN(mc.mp_units, "elu", cfg.dim_emb, mc.num_clusters).to(DEV)         # the caller passes dim_emb, not 9
    clusters = train_clustering(None, dataset, scn, mc, OptimConfig("adam", lr=0.01),
                                TrainingConfig("hscn", "cross_entropy", "ap"), batch_graphs=1)
    assert scn.last_engine == "resident"
    assert len(clusters) == 40 and all(c.shape[0] == g.num_nodes for c, g in zip(clusters, dataset))
    split = {"train": torch.arange(0, 24), "val": torch.arange(24, 32), "test": torch.arange(32, 40)}
    hs = generate_hetero_data(clusters, dataset, split, dc, mc, None)
    model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], cfg.dim_emb, 16, 10, 3).to(DEV)
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=3, eval_period=1, patience=50)
    ev = [DataLoader(hs[24:32], batch_size=8), DataLoader(hs[32:], batch_size=8)]
    hist = fit_resident(None, OptimConfig("adamW", lr=0.01), tc, hs[:24], ev, model, batch_size=8)
    assert len(hist) == 3 and all(np.isfinite(l) for l, _ in hist)
    assert model.last_engine == "resident"
