"""A trainable positional encoder inside GPS and MPNN (``pos_enc``: model/_common.py PosEnc) on a synthetic categorical
batch of eight graphs of 1 to 40 nodes: ``encode_nodes`` against the float64 oracle of the encoder on the statistics
the model used, one epoch through ``train.train``, the statistics cache, the flag words and the refusals."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, CONV_DICT
from graph_hscn.data import Batch, DataLoader
from graph_hscn.loader.synthetic import SHAPES, make_graph
from graph_hscn.train import batching
from tests import lappe_oracle as LO
from tests.helpers import f64_close

DEV = "cuda"
SIZES = [1, 2, 7, 40, 23, 12, 31, 5]
D, DIM_PE, K, KSTEPS = 32, 8, 10, 12
MODELS = ["gps_atom_plain", "gps_published", "mpnn_atom", "mpnn_float"]
KINDS = ["lappe", "rwse"]


def _graphs():
    rng, edge_rng = np.random.default_rng(5), np.random.default_rng(6)
    return [make_graph(rng, SHAPES["peptides_func"], n=n, edge_features=True, edge_rng=edge_rng) for n in SIZES]


def _cfg(kind):
    from graph_hscn.config.config import LapPEConfig, RWSEConfig
    if kind == "lappe":
        return LapPEConfig(dim_in=9, dim_emb=D, dim_pe=DIM_PE, layers=2, post_layers=1, eigen_max_freqs=K)
    return RWSEConfig(dim_in=9, dim_emb=D, dim_pe=DIM_PE, ksteps=KSTEPS, model="mlp", layers=2)


def _model(name, kind, seed=0):
    from graph_hscn.model.gps import GPS
    from graph_hscn.model.mpnn import MPNN
    relu, cfg = ACT_DICT["relu"], _cfg(kind)
    torch.manual_seed(seed)
    if name == "gps_atom_plain":
        m = GPS(9, D, 10, 2, 4, None, relu, node_encoder="atom", pos_enc=cfg)
    elif name == "gps_published":
        m = GPS(9, D, 10, 2, 4, "gatedgcn", relu, node_encoder="atom", edge_encoder="bond", pos_enc=cfg)
    elif name == "mpnn_atom":
        m = MPNN(CONV_DICT["gcn"], relu, 9, D, 10, 3, node_encoder="atom", pos_enc=cfg)
    else:
        m = MPNN(CONV_DICT["gcn"], relu, 9, D, 10, 3, pos_enc=cfg)
    m = m.to(DEV)
    m.pe_encoder.pe_seed = 17                      # (LapPE: the flips of every step; RWSE ignores it)
    return m


def _dense_chain(x, layers, act=True):
    """float64 value and absolute-value magnitude of Linear (+ ReLU) layers, and the bound's n they add."""
    v, mag, n = x.double(), x.double().abs(), 0
    for fc in layers:
        W, b = fc.weight.detach().cpu().double(), fc.bias.detach().cpu().double()
        v, mag = v @ W.t() + b, mag @ W.abs().t() + b.abs()
        if act:
            v = torch.relu(v)
        n += W.shape[1] + 1 + 4
    return v, mag, n


class _CallSpy:
    """Names issued through ``_hip.call`` (the statistics launches of transform/) while active."""

    def __init__(self, monkeypatch):
        self.names = []
        real = _hip.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(_hip, "call", call)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_encode_nodes_is_the_node_encoder_beside_the_oracle_pe(name, kind):
    m = _model(name, kind).eval()
    host = Batch.from_data_list(_graphs())
    b = batching.to_device(m, host, DEV)
    with torch.no_grad():
        h = m.encode_nodes(b)
        own = m._embed_x(b)
    m.check_flags()
    N = sum(SIZES)
    assert h.shape == (N, D) and own.shape == (N, D - DIM_PE)
    assert torch.equal(h[:, :D - DIM_PE], own)
    stats = [t.cpu() for t in m._pe_stats(b)]
    enc = m.pe_encoder
    if kind == "lappe":
        vec, val = stats
        assert vec.shape == (N, K) and bool(torch.isnan(vec[0, 1:]).all()) and not bool(torch.isnan(vec[0, 0]))
        chain = [enc.linear_A] + list(enc.pe_encoder)
        Ws, bs = [f.weight for f in chain], [f.bias for f in chain]
        pe, _, _ = LO.chain(vec, val, Ws, bs, None)
        mag, _, _ = LO.chain(vec, val, Ws, bs, None, absolute=True)
        n = LO.bound_n(DIM_PE, 2, K)
        W, bias = enc.post_mlp[0].weight.detach().cpu().double(), enc.post_mlp[0].bias.detach().cpu().double()
        ref, mag, n = torch.relu(pe @ W.t() + bias), mag @ W.abs().t() + bias.abs(), n + DIM_PE + 1 + 4
        dropped, _, _ = LO.chain(vec, val, Ws, bs, None, drop_freq=0)
        dropped = torch.relu(dropped @ W.t() + bias)
    else:
        (rw,) = stats
        assert rw.shape == (N, KSTEPS)
        ref, mag, n = _dense_chain(rw, enc.pe_encoder)
        rw0 = rw.clone()
        rw0[:, 1] = 0.0                            # the tooth: the two-step return probability left out
        dropped, _, _ = _dense_chain(rw0, enc.pe_encoder)
    assert f64_close(h[:, D - DIM_PE:], ref, mag, n, what=f"{name} {kind} pe")
    assert not f64_close(h[:, D - DIM_PE:], dropped, mag, n), "the bound cannot see a dropped input column"


def _train_once(name, kind, epochs=1, loaders=None):
    from graph_hscn.train.train import train
    m = _model(name, kind, seed=3)
    grads = {}
    for pname, p in m.named_parameters():
        if pname.startswith(("pe_encoder.", "linear_x.")):
            p.register_hook(lambda g, pname=pname: grads.setdefault(pname, []).append(g.detach().clone()))
    graphs = _graphs()
    if loaders is None:
        loaders = [DataLoader(graphs, 4), DataLoader(graphs, 8)]
    cfg = SimpleNamespace(model_type="gps", epochs=epochs, eval_period=1, loss_fn="cross_entropy", patience=10,
                          min_delta=0.0, metric="ap")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    history = train(None, opt, cfg, loaders, m)
    torch.cuda.synchronize()
    return m, grads, history


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MODELS)
def test_one_epoch_trains_the_encoder_and_two_runs_agree_bitwise(name, kind):
    m1, grads, history = _train_once(name, kind)
    assert len(history) == 1 and np.isfinite(history[0][0])
    names = [n for n, _ in m1.named_parameters() if n.startswith("pe_encoder.")]
    assert names
    for n in names:
        assert n in grads and len(grads[n]) == 2, n                       # two batches of four graphs
        for g in grads[n]:
            assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, n
    m2, grads2, history2 = _train_once(name, kind)
    assert [h[0] for h in history] == [h[0] for h in history2]
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for n in names:
        assert all(torch.equal(a, b) for a, b in zip(grads[n], grads2[n])), n


@pytest.mark.gpu
@pytest.mark.parametrize("kind,entry", [("lappe", "hscn_lap_eig_stats"), ("rwse", "hscn_rwse_stats")])
def test_the_statistics_of_a_reused_batch_are_computed_once(kind, entry, monkeypatch):
    graphs = _graphs()
    batches = [Batch.from_data_list(graphs[:4]), Batch.from_data_list(graphs[4:])]
    spy = _CallSpy(monkeypatch)
    m, _, history = _train_once("mpnn_atom", kind, epochs=2, loaders=[batches, batches[:1]])
    assert len(history) == 2
    assert spy.names.count(entry) == 2             # one launch per loader batch: two epochs and two evaluations reuse them
    # a batch that carries the statistics at the configured width is not decomposed at all
    host = Batch.from_data_list(graphs[:4])
    b = batching.to_device(m, host, DEV)
    if kind == "lappe":
        b.eigvecs_sn, b.eigvals_sn = torch.randn(b.num_nodes, K, device=DEV), torch.rand(b.num_nodes, K, 1, device=DEV)
    else:
        b.rwse = torch.rand(b.num_nodes, KSTEPS, device=DEV)
    before = spy.names.count(entry)
    with torch.no_grad():
        m.eval()(b)
    assert spy.names.count(entry) == before


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["gps_atom_plain", "mpnn_float"])
def test_an_edge_outside_its_graph_is_reported_by_check_flags_not_by_forward(name, kind):
    m = _model(name, kind).eval()
    host = Batch.from_data_list(_graphs())
    ei = host.edge_index.clone()
    e = int(host.eptr32[3])                        # the first edge of graph 3 now ends in graph 2
    ei[1, e] = int(host.ptr[2])
    host.edge_index = ei
    b = batching.to_device(m, host, DEV)
    with torch.no_grad():
        out = m(b)                                 # nothing is read back here
    assert out.shape == (len(SIZES), 10)
    with pytest.raises(RuntimeError, match="an edge with an end outside its graph"):
        m.check_flags()
    m.check_flags()                                # reported once: the word is consumed


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gps_published", "mpnn_float"])
def test_resident_entry_points_refuse_with_the_models_own_reason(name):
    import re

    from graph_hscn.replay import CapturedStep
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    m = _model(name, "lappe")
    reason = m.resident_reason()
    assert "positional encoder" in reason and m.layered_only
    graphs = _graphs()
    bd = batching.to_device(m, Batch.from_data_list(graphs[:4]), DEV)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        fit_resident(None, opt, cfg, graphs, [], m, 4)
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        CapturedStep(m, SimpleNamespace(batch=bd), "cross_entropy")
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        DeviceEvaluator(graphs, m, "cross_entropy", 4).run()
    m.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="positional encoder"):
        m(bd)


@pytest.mark.gpu
def test_compute_posenc_with_a_lappe_config_is_a_frozen_pre_stage():
    from graph_hscn.train.train import compute_posenc
    graphs = _graphs()
    for g in graphs:
        g.x = g.x.float()
    cfg = _cfg("lappe")
    data_cfg = SimpleNamespace(batch_size=4)

    def run(stats):
        torch.manual_seed(8)
        loaders, flat = compute_posenc([DataLoader(graphs, 4)], data_cfg, 9, cfg, device=DEV, stats=stats)
        return torch.cat([b.x for b in flat]).cpu(), loaders

    x1, loaders = run(None)
    x2, _ = run("device")
    assert x1.shape == (sum(SIZES), D) and bool(torch.isfinite(x1).all())
    assert torch.equal(x1, x2)                     # eval mode: no flips, whatever the host seed counter says
    enc = compute_posenc.last_encoder
    assert type(enc).__name__ == "LapPENodeEncoder" and not enc.training
    assert sum(b.x.size(0) for b in loaders[0]) == sum(SIZES)
    assert float(x1[:, D - DIM_PE:].abs().max()) > 0.0
