"""SAN without a device: config and constructor validation, every refusal that happens before a launch, parameter names,
the C ABI's additions, the envelope function at its edges and the restatement's own properties (tests/san_oracle.py)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, LapPEConfig, SANConfig
from graph_hscn.data import Batch, Data
from graph_hscn.model import san as san_model
from graph_hscn.model.san import SAN, build_san
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import SANAttention
from graph_hscn.nn.san import SANLayer
from tests import san_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hscn_san_attn_supported", "hscn_san_attn_fwd", "hscn_san_attn_bwd_dst", "hscn_san_attn_bwd_src")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_abi_stays_24_and_the_new_symbols_are_declared_and_bound():
    L = _hip.lib()
    assert L.hscn_abi_version() == 24 == _hip.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hscn.h")).read(), flags=re.S)
    assert "#define HSCN_ABI_VERSION 24" in header
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _hip.exported_symbols() and hasattr(L, name)


def test_supported_at_its_edges():
    L = _hip.lib()
    ok = L.hscn_san_attn_supported
    assert ok(1, 4, 0) and ok(8, 64, 4096) and ok(128, 4, 1) and ok(3, 12, 97) and ok(1, 64, 4096)
    assert not ok(1, 0, 8) and not ok(1, 2, 8) and not ok(1, 6, 8) and not ok(1, 68, 8)      # C a multiple of 4 in [4, 64]
    assert not ok(0, 4, 8) and not ok(-1, 4, 8)
    assert ok(8, 64, 8) and not ok(9, 64, 8) and not ok(129, 4, 8) and ok(32, 16, 8) and not ok(33, 16, 8)   # HC <= 512
    assert not ok(4, 8, -1) and not ok(4, 8, 4097)
    assert Fh.SAN_MAX_NODES == 4096 and Fh.san_attn_supported(4, 8, 4096) and not Fh.san_attn_supported(4, 8, 4097)
    assert Fh.san_attn_supported(4, 8) and "4096" in Fh.SAN_ENVELOPE and "512" in Fh.SAN_ENVELOPE


def test_entry_points_refuse_before_any_launch():
    L = _hip.lib()
    one = 16                                       # (a non-NULL, 16-byte aligned address that is never dereferenced)
    tail = lambda N, E, B, mx, h, c, g, full: (N, E, B, mx, h, c, g, full, one, None)
    fwd = lambda ptrs, *t: L.hscn_san_attn_fwd(*ptrs, *tail(*t))
    P12 = [one] * 12
    assert fwd(P12, 4, 4, 1, 8, 2, 6, 0.1, 1) == -3                      # head width
    assert fwd(P12, 4, 4, 1, 8, 9, 64, 0.1, 1) == -3                     # heads * C > 512
    assert fwd(P12, 4, 4, 1, 4097, 2, 8, 0.1, 1) == -3                   # beyond the bitset envelope
    assert fwd(P12, -1, 4, 1, 8, 2, 8, 0.1, 1) == -1
    assert fwd(P12, 4, 4, 1, 8, 2, 8, -0.5, 1) == -1                     # gamma < 0
    assert fwd(P12, 4, 4, 1, 8, 2, 8, float("nan"), 1) == -1
    assert fwd(P12, 4, 4, 1, 8, 2, 8, float("inf"), 1) == -1
    assert fwd(P12, 0, 0, 0, 8, 2, 8, 0.1, 1) == 0                       # nothing to do
    no_q2 = [one] * 8 + [None, one, one, one]
    assert fwd(no_q2, 4, 4, 1, 8, 2, 8, 0.1, 1) == -1                    # full_graph without q2
    no_e = [one] * 7 + [None] + [one] * 4
    assert fwd(no_e, 4, 4, 1, 8, 2, 8, 0.1, 1) == -1                     # edges without e
    odd = [one] * 4 + [20] + [one] * 7
    assert fwd(odd, 4, 4, 1, 8, 2, 8, 0.1, 1) == -1                      # q not 16-byte aligned
    assert L.hscn_san_attn_bwd_dst(*([one] * 17), *tail(4, 4, 1, 8, 2, 8, 0.1, 0)) == -1     # dq2 without full_graph
    assert L.hscn_san_attn_bwd_src(*([one] * 16), *tail(4, 4, 1, 8, 2, 8, 0.1, 0)) == -1     # dk2e without full_graph
    assert L.hscn_san_attn_bwd_src(*([one] * 13), None, None, None, *tail(4, 4, 1, 8, 2, 8, 0.1, 1)) == 0   # nothing asked
    assert L.hscn_san_attn_bwd_dst(*([one] * 17), *tail(4, 4, 1, 8, 2, 5, 0.1, 1)) == -3


# ---- config and constructors -------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    cfg = SANConfig("relu")
    assert (cfg.gamma, cfg.full_graph, cfg.num_heads, cfg.norm, cfg.task_level) == (1e-1, True, 4, "layer", "graph")
    assert (cfg.node_encoder, cfg.edge_encoder, cfg.pos_enc, cfg.pe_undirected) == (None, None, None, True)
    for kw, match in ((dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("inf")), "gamma"),
                      (dict(task_level="edge"), "task_level"), (dict(norm="group"), "norm"),
                      (dict(node_encoder="ast"), "node_encoder"), (dict(edge_encoder="ast"), "edge_encoder"),
                      (dict(hidden_channels=18), "divisible"), (dict(hidden_channels=8, num_heads=4), "head width"),
                      (dict(hidden_channels=1024, num_heads=16), "512"), (dict(full_graph=1), "full_graph"),
                      (dict(activation="swish"), "activation"), (dict(num_layers=0), "positive"),
                      (dict(pos_enc=LapPEConfig(9, 32, 8), hidden_channels=16), "dim_emb")):
        args = dict(activation="relu", hidden_channels=16)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            SANConfig(**args)
    assert SANConfig("relu", gamma=0).gamma == 0 and SANConfig("relu", gamma=4).gamma == 4
    for key in ("gamma_learn", "attn_dropout"):                 # not built, and not configurable: the constructors refuse
        with pytest.raises(TypeError):
            SANConfig("relu", **{key: True})
    m = build_san(SANConfig("relu", hidden_channels=16, num_layers=2, node_encoder="atom", edge_encoder="bond",
                            gamma=0.25, pos_enc=LapPEConfig(9, 16, 4), task_level="node"), 9, 3)
    assert (m.gamma, m.full_graph, m.task_level, m.num_layers) == (0.25, True, "node", 2)
    assert tuple(m.node_encoder.weight.shape)[1] == 12 and tuple(m.edge_encoder.weight.shape)[1] == 16
    assert all(layer.attention.gamma == 0.25 for layer in m.layers)


def test_constructor_refusals_by_name():
    kw = dict(num_features=9, hidden_channels=16, num_classes=3, num_layers=1, num_heads=4)
    with pytest.raises(ValueError, match="gamma"):
        SAN(**kw, gamma=-1.0)
    with pytest.raises(ValueError, match="gamma"):
        SAN(**kw, gamma=float("inf"))
    with pytest.raises(NotImplementedError, match="gamma_learn"):
        SAN(**kw, gamma_learn=True)
    with pytest.raises(NotImplementedError, match="dropout on the attention weights"):
        SAN(**kw, attn_dropout=0.1)
    with pytest.raises(NotImplementedError, match="gamma_learn"):
        SANLayer(16, 4, gamma_learn=True)
    with pytest.raises(NotImplementedError, match="dropout on the attention weights"):
        SANAttention(16, 4, attn_dropout=0.5)
    with pytest.raises(ValueError, match="envelope"):
        SANAttention(24, 4)                                     # head width 6
    with pytest.raises(ValueError, match="envelope"):
        SANAttention(1024, 16)                                  # wider than 512
    with pytest.raises(ValueError, match="multiple of num_heads"):
        SANAttention(18, 4)
    with pytest.raises(ValueError, match="norm"):
        SANLayer(16, 4, norm="group")
    with pytest.raises(ValueError, match="task_level"):
        SAN(**kw, task_level="edge")
    with pytest.raises(ValueError, match="at least one layer"):
        SAN(9, 16, 3, 0)


def test_parameter_names_and_state_dict_keys():
    att = SANAttention(16, 4)
    assert [n for n, _ in att.named_parameters()] == [f"{p}.weight" for p in ("Q", "K", "E", "Q_2", "K_2", "E_2", "V")]
    assert all(tuple(p.shape) == (16, 16) for p in att.parameters())
    assert [n for n, _ in SANAttention(16, 4, full_graph=False).named_parameters()] == ["Q.weight", "K.weight", "E.weight",
                                                                                      "V.weight"]
    m = SAN(9, 16, 3, 1, 4, edge_encoder="bond")
    layer = ["attention.Q.weight", "attention.K.weight", "attention.E.weight", "attention.Q_2.weight",
             "attention.K_2.weight", "attention.E_2.weight", "attention.V.weight", "O_h.weight", "O_h.bias",
             "norm1_h.weight", "norm1_h.bias", "FFN_h_layer1.weight", "FFN_h_layer1.bias", "FFN_h_layer2.weight",
             "FFN_h_layer2.bias", "norm2_h.weight", "norm2_h.bias"]
    assert list(m.state_dict().keys()) == (["node_encoder.weight", "node_encoder.bias", "edge_encoder.weight",
                                            "fake_edge_emb.weight"] + ["layers.0." + k for k in layer]
                                           + ["lin_1.weight", "lin_1.bias", "lin_2.weight", "lin_2.bias"])
    assert tuple(m.fake_edge_emb.weight.shape) == (1, 16)
    plain = SAN(9, 16, 3, 1, 4, edge_encoder="bond", full_graph=False)
    assert not any("_2.weight" in k and "attention" in k or "fake" in k for k in plain.state_dict())
    # the restatement has the same keys: weights move both ways
    ref = SO.SANRef(9, 16, 3, 1, 4, edge_encoder=(5, 6, 2))
    assert list(ref.state_dict().keys()) == list(m.state_dict().keys())
    m.load_state_dict(ref.state_dict(), strict=True)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _cpu_batch(edge_attr=True):
    g = torch.Generator().manual_seed(0)
    graphs = []
    for n in (5, 7):
        d = Data(x=torch.randn(n, 9, generator=g), edge_index=torch.randint(0, n, (2, 2 * n), generator=g),
                 y=torch.zeros(1, 3))
        if edge_attr:
            d.edge_attr = torch.randn(2 * n, 3, generator=g)
        graphs.append(d)
    return Batch.from_data_list(graphs)


def test_the_operator_refuses_before_any_launch():
    b = _cpu_batch()
    N, E = 12, 24
    rel = SimpleNamespace(num_edges=E, num_src=N, num_dst=N)
    q, e = torch.randn(N, 16), torch.randn(E, 16)
    run = lambda *a, **k: Fh.SANAttentionFn.apply(*a)
    full = (q, q, q, e, q, q, rel, b.ptr32, 7, 4)
    with pytest.raises(RuntimeError, match="HIP device tensors only"):
        run(*full, 0.1, True)
    with pytest.raises(ValueError, match="gamma"):
        run(*full, -0.1, True)
    with pytest.raises(ValueError, match="gamma"):
        run(*full, float("nan"), True)
    with pytest.raises(TypeError, match="float32"):
        run(q.double(), q, q, e, q, q, rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(ValueError, match="one row per edge"):
        run(q, q, q, e[:-1], q, q, rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(ValueError, match="e is None"):
        run(q, q, q, None, q, q, rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(ValueError, match="full_graph needs q2"):
        run(q, q, q, e, None, None, rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(ValueError, match="belong to full_graph=True"):
        run(q, q, q, e, q, q, rel, b.ptr32, 7, 4, 0.1, False)
    with pytest.raises(ValueError, match="envelope"):
        run(q, q, q, e, q, q, rel, b.ptr32, 7, 8, 0.1, True)                 # head width 2
    with pytest.raises(ValueError, match="envelope"):
        run(*full[:8], 4097, 4, 0.1, True)                                   # a graph beyond the bitset
    with pytest.raises(ValueError, match="k2e is"):
        run(q, q, q, e, q, q[:-1], rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(ValueError, match="relation"):
        run(q[:-1], q[:-1], q[:-1], e, q[:-1], q[:-1], rel, b.ptr32, 7, 4, 0.1, True)
    with pytest.raises(TypeError, match="ptr32"):
        run(*full[:7], b.ptr32.long(), 7, 4, 0.1, True)
    with pytest.raises(RuntimeError, match="HIP device tensors only"):       # gamma is not read without full_graph
        run(q, q, q, e, None, None, rel, b.ptr32, 7, 4, -1.0, False)


def test_a_batch_without_edge_attr_and_cpu_tensors_are_refused():
    m = SAN(9, 16, 3, 1, 4)
    with pytest.raises(ValueError, match="carries no edge_attr"):
        m(_cpu_batch(edge_attr=False))
    with pytest.raises(RuntimeError, match="HIP device tensors only|CPU tensor"):
        m(_cpu_batch())
    att = SANAttention(16, 4)
    with pytest.raises(ValueError, match="needs edge_attr"):
        att(torch.randn(12, 16), _cpu_batch().edge_index, None, _cpu_batch(), torch.randn(1, 16))
    with pytest.raises(ValueError, match="one row per edge"):
        att(torch.randn(12, 16), _cpu_batch().edge_index, torch.randn(5, 16), _cpu_batch(), torch.randn(1, 16))


def test_every_resident_entry_point_refuses_the_model_with_its_own_reason():
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    m = SAN(9, 16, 3, 1, 4, ACT_DICT["relu"])
    reason = m.resident_reason()
    assert m.layered_only and not m.supported() and reason == san_model.RESIDENT_REASON and "SAN" in reason
    assert "positional encoder" in SAN(9, 16, 3, 1, 4, pos_enc=LapPEConfig(9, 16, 4)).resident_reason()
    assert "edge_encoder='bond'" in SAN(9, 16, 3, 1, 4, edge_encoder="bond").resident_reason()
    b = _cpu_batch()
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        fit_resident(None, opt, cfg, [], [], m, 4)
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        DeviceEvaluator([], m, "cross_entropy", 4)
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        batching.resident_step(m, b, "cross_entropy")
    from graph_hscn.step import MPNNResidentTrainStep
    with pytest.raises(RuntimeError, match=re.escape(reason)):
        MPNNResidentTrainStep(m, b, "cross_entropy")
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="SAN's attention over real and fake edges"):
        m(b)
    m.engine = "captured"
    with pytest.raises(ValueError, match="engine"):
        m(b)


# ---- the restatement's own properties ---------------------------------------------------------------------------------
def _rand(N, E, heads, C, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda r: torch.randn(r, heads * C, generator=g, dtype=dtype)
    return dict(q=mk(N), k=mk(N), v=mk(N), e=mk(E), q2=mk(N), k2e=mk(N))


def _att(x, ei, ptr, heads, gamma=0.1, full=True, skip=None):
    q2, k2e = (x["q2"], x["k2e"]) if full else (None, None)
    return SO.attention(x["q"], x["k"], x["v"], x["e"], q2, k2e, ei, ptr, heads, gamma, full, skip)


def test_gamma_zero_is_the_real_term_alone():
    ei = torch.tensor([[0, 1, 2, 2, 4, 5], [1, 0, 0, 2, 5, 4]])
    ptr, x = [0, 4, 6], _rand(6, 6, 2, 4, 1)                    # node 3 has no in-edge
    out0, z0 = _att(x, ei, ptr, 2, gamma=0.0)
    out1, z1 = _att(x, ei, ptr, 2, full=False)
    assert torch.equal(out0, out1) and torch.equal(z0, z1)      # a = 1, b = 0: the fake terms are exact zeros
    assert not out0[3].any() and not z0[3].any()                # and 0 / (0 + 1e-6) = 0
    w = torch.exp(((x["q"][1] * x["k"][0] * x["e"][0]).view(2, 4).sum(-1) / 2.0).clamp(-5, 5))
    assert torch.allclose(z0[1], w) and torch.allclose(out0[1].view(2, 4), w[:, None] * x["v"][0].view(2, 4) / (w + 1e-6)[:, None])


def test_a_complete_graph_with_self_loops_has_no_fake_pair():
    n = 4
    ei = torch.tensor([[j for j in range(n) for i in range(n)], [i for j in range(n) for i in range(n)]])
    x = _rand(n, n * n, 2, 4, 2)
    _, _, s_real, s_fake = SO.attention(x["q"], x["k"], x["v"], x["e"], x["q2"], x["k2e"], ei, [0, n], 2, 0.5, True,
                                        want_scores=True)
    assert tuple(s_real.shape) == (n * n, 2) and s_fake.numel() == 0
    out, z = _att(x, ei, [0, n], 2, gamma=0.5)
    out_r, z_r = _att(x, ei, [0, n], 2, full=False)
    assert torch.allclose(z, z_r / 1.5) and torch.allclose(out, out_r, atol=1e-6)      # Z_fake = 0: only a differs
    moved = dict(x, q2=x["q2"] * 3.0, k2e=x["k2e"] - 1.0)
    assert torch.equal(_att(moved, ei, [0, n], 2, gamma=0.5)[0], out)


def test_an_edgeless_graph_has_only_fake_pairs_the_diagonal_included():
    n = 3
    ei = torch.zeros(2, 0, dtype=torch.long)
    x = _rand(n, 0, 2, 4, 3)
    _, z, s_real, s_fake = SO.attention(x["q"], x["k"], x["v"], x["e"], x["q2"], x["k2e"], ei, [0, n], 2, 1.0, True,
                                        want_scores=True)
    assert s_real.numel() == 0 and tuple(s_fake.shape) == (n * n, 2)
    s = (x["q2"].view(n, 1, 2, 4) * x["k2e"].view(1, n, 2, 4)).sum(-1) / 2.0                # [i, j, h]
    assert torch.allclose(z, 0.5 * torch.exp(s.clamp(-5, 5)).sum(1))
    out, _ = _att(x, ei, [0, n], 2, gamma=1.0)
    assert float((_att(x, ei, [0, n], 2, gamma=1.0, skip=("fake", (1, 1)))[0] - out)[1].abs().max()) > 1e-6   # the diagonal counts


def test_direction_and_duplicates():
    ei = torch.tensor([[0, 0, 0, 2], [1, 1, 2, 0]])              # 0 -> 1 twice, 0 -> 2, 2 -> 0
    x = _rand(3, 4, 2, 4, 4)
    _, _, s_real, s_fake = SO.attention(x["q"], x["k"], x["v"], x["e"], x["q2"], x["k2e"], ei, [0, 3], 2, 0.1, True,
                                        want_scores=True)
    assert s_real.size(0) == 4 and s_fake.size(0) == 9 - 3       # (0,1), (0,2), (2,0) are real; (1,0), (1,2), (2,1), diag fake
    out, z = _att(x, ei, [0, 3], 2)
    out_d, z_d = _att(x, ei, [0, 3], 2, skip=("real", 1))        # the last edge of the duplicated pair
    assert float((out_d - out)[1].abs().max()) > 1e-6 and float((z - z_d)[1].min()) > 0
    assert torch.equal(out_d[0], out[0]) and torch.equal(out_d[2], out[2])
    # dropping it leaves the pair real: no fake term appears in its place
    only = torch.tensor([[0, 0, 2], [1, 2, 0]])
    x1 = dict(x, e=x["e"][[0, 2, 3]])
    assert torch.allclose(_att(x1, only, [0, 3], 2)[0], out_d) and torch.allclose(_att(x1, only, [0, 3], 2)[1], z_d)
    # an edge between two graphs is in neither
    cross = torch.tensor([[0, 3], [1, 1]])
    xc = _rand(5, 2, 2, 4, 5)
    a = _att(xc, cross, [0, 3, 5], 2)
    bb = _att(dict(xc, e=xc["e"][:1]), cross[:, :1], [0, 3, 5], 2)
    assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])
