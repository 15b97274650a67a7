"""GatedGCN without a GPU: the registry and the configs take "gatedgcn", the modules carry GraphGPS's parameter names and
load the restatement's ``state_dict``, the lazily sized pieces are sized by what they first see, every place that cannot
run the convolution refuses it by name, existing models keep their ``state_dict`` keys, the entry points check their
arguments before any launch, and the float64 restatement (tests/gatedgcn_oracle.py) satisfies the identities and the
hand-written backward formulas the kernels implement."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from graph_hscn.config.config import ACT_DICT, CONV_DICT, GPSConfig, MPNNConfig
from graph_hscn.data import Batch
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.conv import GatedGCNConv, GatedGCNLayer, Linear
from graph_hscn.nn.gps import GPSLayer
from graph_hscn.nn.norm import BatchNorm1d, LayerNorm
from tests import gatedgcn_oracle as GG

UNINIT = torch.nn.parameter.UninitializedParameter


# --------------------------------------------------------------------------- #
# 1. registry, configs, parameter names
# --------------------------------------------------------------------------- #
def test_registry_and_configs_take_gatedgcn():
    assert CONV_DICT["gatedgcn"] is GatedGCNConv
    assert GatedGCNConv.uses_edge_attr is True and GatedGCNConv.updates_edge_attr is True
    cfg = GPSConfig("relu", local_conv_type="gatedgcn")
    assert cfg.local_conv_type == "gatedgcn"
    assert GPSConfig("relu").local_conv_type == "gine"                      # the default stays
    m = build_gps(GPSConfig("relu", "GatedGCN", 16, 2, 4, 0.0), 9, 10)
    assert all(type(layer.conv) is GatedGCNLayer and layer.updates_edge_attr and layer.uses_edge_attr for layer in m.layers)
    assert isinstance(m.edge_encoder, Linear) and m.edge_encoder.out_channels == 16
    b = build_mpnn(MPNNConfig("gatedgcn", "relu"), 9, 10)
    assert len(b.conv_layers) == 3 and all(type(c) is GatedGCNConv for c in b.conv_layers)
    assert [(c.A.in_channels, c.A.out_channels) for c in b.conv_layers] == [(9, 16), (16, 16), (16, 10)]
    assert [c.C.out_channels for c in b.conv_layers] == [16, 16, 10]


def test_state_dict_keys_are_graphgps_names_and_load_from_the_restatement():
    torch.manual_seed(0)
    conv = GatedGCNConv(9, 16, edge_dim=3)
    ref = GG.GatedGCNConvRef(9, 16, 3)
    assert [n for n, _ in conv.named_parameters()] == [f"{m}.{p}" for m in "ABCDE" for p in ("weight", "bias")]
    assert list(conv.state_dict()) == list(ref.state_dict())
    conv.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(conv.state_dict()[k], v) for k, v in ref.state_dict().items())
    layer = GatedGCNLayer(16, dropout=0.1, edge_dim=16)
    lref = GG.GatedGCNLayerRef(16)
    assert list(layer.state_dict()) == list(lref.state_dict())
    assert {k.split(".")[0] for k in layer.state_dict()} == {"A", "B", "C", "D", "E", "bn_node_x", "bn_edge_e"}
    layer.load_state_dict(lref.state_dict(), strict=True)
    assert isinstance(layer.bn_node_x, BatchNorm1d) and isinstance(layer.bn_edge_e, BatchNorm1d)
    assert isinstance(GatedGCNLayer(16, norm="layer").bn_edge_e, LayerNorm) and GatedGCNLayer(16, norm=None).bn_node_x is None
    # the models
    mref = GG.GatedGCNModelRef(9, 16, 10, 3, 3)
    model = MPNN(CONV_DICT["gatedgcn"], ACT_DICT["relu"], 9, 16, 10, 3)
    for i, d in enumerate((3, 16, 16)):
        assert isinstance(model.conv_layers[i].C.weight, UNINIT)
        model.conv_layers[i].C.materialize(d, torch.zeros(1))
    assert set(model.state_dict()) == set(mref.state_dict())
    model.load_state_dict(mref.state_dict(), strict=True)
    gref = GG.GatedGPSRef(9, 16, 10, 2, 4, edge_dim=3)
    gps = GPS(9, 16, 10, 2, num_heads=4, local_conv="gatedgcn")
    assert isinstance(gps.edge_encoder.weight, UNINIT)
    gps.edge_encoder.materialize(3, torch.zeros(1))
    for layer in gps.layers:
        layer.conv.C.materialize(16, torch.zeros(1))
    assert set(gps.state_dict()) == set(gref.state_dict())
    gps.load_state_dict(gref.state_dict(), strict=True)


def test_lazy_sizing_of_c_and_the_edge_encoder():
    conv = GatedGCNConv(9, 16)
    assert isinstance(conv.C.weight, UNINIT) and conv.A.weight.shape == (16, 9)
    assert GatedGCNConv(9, 16, edge_dim=5).C.weight.shape == (16, 5)
    conv.C.materialize(7, torch.zeros(1))
    assert conv.C.weight.shape == (16, 7) and conv.C.in_channels == 7
    # sized by the edge features the module first sees: the launch that would follow has no CPU form
    conv = GatedGCNConv(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.randn(5, 4), torch.randint(0, 5, (2, 6)), torch.randn(6, 3))
    assert conv.C.weight.shape == (8, 3)


def test_existing_models_keep_their_state_dict_keys():
    gps = GPS(9, 16, 10, 2, num_heads=4, local_conv="gine")
    per_layer = ["conv.eps", "conv.nn.0.weight", "conv.nn.0.bias", "conv.nn.2.weight", "conv.nn.2.bias", "conv.lin.weight",
                 "conv.lin.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                 "attn.out_proj.bias", "norm1_local.weight", "norm1_local.bias", "norm1_attn.weight", "norm1_attn.bias",
                 "ff_linear1.weight", "ff_linear1.bias", "ff_linear2.weight", "ff_linear2.bias", "norm2.weight",
                 "norm2.bias"]
    want = {"node_encoder.weight", "node_encoder.bias", "lin_1.weight", "lin_1.bias", "lin_2.weight", "lin_2.bias"}
    want |= {f"layers.{i}.{k}" for i in range(2) for k in per_layer}
    assert set(gps.state_dict()) == want and not hasattr(gps, "edge_encoder")
    for conv in ("gcn", "gat", None):
        assert not any("edge_encoder" in k for k in GPS(9, 16, 10, 1, 4, conv).state_dict())
    gine = build_mpnn(MPNNConfig("gine", "relu"), 9, 10)
    assert set(gine.state_dict()) == {f"conv_layers.{i}.{k}" for i in range(3) for k in (
        "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "lin.weight", "lin.bias", "eps")}
    # a layer without an edge-updating convolution still returns a Tensor-typed surface
    assert not GPSLayer(16, "gine", 4).updates_edge_attr and not GPSLayer(16, None, 4).updates_edge_attr


# --------------------------------------------------------------------------- #
# 2. refusals by name
# --------------------------------------------------------------------------- #
def test_refusals_by_name():
    from graph_hscn.model.hscn import HSCN, build_conv_relation
    from graph_hscn.train import batching
    with pytest.raises(ValueError, match="'GatedGCN' needs edge features"):
        build_conv_relation("GatedGCN", 16)
    with pytest.raises(ValueError, match="'GatedGCN' needs edge features"):
        HSCN("GAT", "gatedgcn", "GCN", ACT_DICT["relu"], 9, 16, 10, 3)
    # missing and mistyped edge_attr, models and modules
    model = build_mpnn(MPNNConfig("gatedgcn", "relu"), 9, 10)
    plain = batching.to_device(model, Batch.from_data_list(make_dataset("peptides_func", 2, 0)), "cpu")
    with pytest.raises(ValueError, match="conv_type 'gatedgcn'.*carries no edge_attr"):
        model(plain)
    ints = Batch.from_data_list(make_dataset("peptides_func", 2, 0, edge_features=True))
    ints.x = ints.x.float()
    with pytest.raises(TypeError, match="float32"):
        model(ints)
    gps = GPS(9, 16, 10, 1, 4, "gatedgcn")
    with pytest.raises(ValueError, match=r"local_conv 'gatedgcn'.*carries no\s+edge_attr"):
        gps(plain)
    with pytest.raises(TypeError, match="float32"):
        gps(ints)
    layer = GPSLayer(16, "gatedgcn", 4)
    monkey_attn = lambda x, batch, ptr32=None, max_nodes=None: x          # noqa: E731  (the attention has no CPU form)
    layer.attn.forward = monkey_attn
    layer.norm1_attn = None
    with pytest.raises(ValueError, match="local_conv 'gatedgcn' needs edge_attr"):
        layer(torch.randn(5, 16), torch.randint(0, 5, (2, 6)), ptr32=torch.tensor([0, 5], dtype=torch.int32), max_nodes=5)
    conv = GatedGCNConv(4, 8, edge_dim=3)
    x, ei = torch.randn(5, 4), torch.randint(0, 5, (2, 6))
    with pytest.raises(ValueError, match="GatedGCNConv needs edge_attr"):
        conv(x, ei, None)
    with pytest.raises(ValueError, match=r"\[E, edge_dim\]"):
        conv(x, ei, torch.randn(6))
    with pytest.raises(TypeError, match="GatedGCNConv: edge_attr must be float32"):
        conv(x, ei, torch.zeros(6, 3, dtype=torch.int64))
    # the envelope, by name, before anything touches the device
    assert [Fh.gatedgcn_supported(h) for h in (0, 1, 512, 513)] == [False, True, True, False]
    with pytest.raises(ValueError, match=r"GatedGCNConv: width H=513 outside the kernel's envelope \(1 <= H <= 512\)"):
        GatedGCNConv(4, 513, edge_dim=3)(x, ei, torch.randn(6, 3))
    with pytest.raises(ValueError, match=r"GatedGCNConv: width H=513 outside"):
        Fh.GatedGCNAggregateFn.apply(*(torch.randn(5, 513) for _ in range(4)), torch.randn(6, 513), None)
    with pytest.raises(TypeError, match="float32"):
        Fh.GatedGCNAggregateFn.apply(*(torch.randn(5, 8).double() for _ in range(4)), torch.randn(6, 8), None)
    rel = SimpleNamespace(num_src=5, num_dst=5, num_edges=6)
    ok = [torch.randn(5, 8) for _ in range(4)]
    with pytest.raises(ValueError, match=r"GatedGCNConv: Dx is \(4, 8\)"):
        Fh.GatedGCNAggregateFn.apply(ok[0], ok[1], torch.randn(4, 8), ok[3], torch.randn(6, 8), rel)
    with pytest.raises(ValueError, match="the relation is 5 -> 5 nodes, x has 7 rows"):
        Fh.GatedGCNAggregateFn.apply(*(torch.randn(7, 8) for _ in range(4)), torch.randn(6, 8), rel)
    with pytest.raises(ValueError, match=r"Ce is \(5, 8\); the relation has 6 edges"):
        Fh.GatedGCNAggregateFn.apply(*ok, torch.randn(5, 8), rel)
    with pytest.raises(ValueError, match=r"Ce is \(6, 4\)"):
        Fh.GatedGCNAggregateFn.apply(*ok, torch.randn(6, 4), rel)
    with pytest.raises(ValueError, match="dropout must be"):
        GatedGCNLayer(16, dropout=1.0)
    with pytest.raises(ValueError, match="norm must be"):
        GatedGCNLayer(16, norm="instance")


def test_resident_entry_points_refuse_the_gatedgcn_baseline_before_anything_is_launched():
    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    m = build_mpnn(MPNNConfig("gatedgcn", "relu", dropout=0.0), 9, 10)         # on the CPU: nothing can launch
    reason = m.resident_reason()
    assert reason.startswith("convolution GatedGCNConv") and not m.supported()
    graphs = make_dataset("peptides_func", 4, seed=0, edge_features=True)
    b = batching.to_device(m, Batch.from_data_list(graphs), "cpu")
    m.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        m(b)
    m.engine = "layered"
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        MPNNResidentTrainStep(m, b, "cross_entropy")
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv"):
        batching.resident_step(m, b, "cross_entropy")              # what replay.CapturedStep builds its step with
    # (the evaluator and fit_resident ask for a HIP device first; on one it names the convolution: tests/test_gpu_gatedgcn.py)
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv|HIP path"):
        DeviceEvaluator(graphs, m, "cross_entropy", 4)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="convolution GatedGCNConv|HIP path"):
        fit_resident(None, opt, cfg, graphs, [], m, 4)


# --------------------------------------------------------------------------- #
# 3. entry points, without a launch
# --------------------------------------------------------------------------- #
def test_entry_points_check_their_arguments_before_any_launch():
    from graph_hscn import _hip
    lib = _hip.lib()
    assert [lib.hscn_gatedgcn_supported(h) for h in (1, 512, 513, 0, -4)] == [1, 1, 0, 0, 0]
    assert lib.hscn_gatedgcn_long_row() == Fh.GATEDGCN_LONG_ROW and lib.hscn_gatedgcn_chunk() == Fh.GATEDGCN_CHUNK
    assert Fh.GATEDGCN_MAX_WIDTH == 512 == Fh.GINE_MAX_WIDTH
    buf = ctypes.create_string_buffer(64)
    here = ctypes.addressof(buf)            # a host buffer standing in for a pointer the checks only compare with NULL
    BADARG, UNSUPPORTED = -1, -3

    def fwd(N, E, H, p=here, edge=here):
        return lib.hscn_gatedgcn_fwd(p, edge, edge, edge, p, p, p, p, edge, p, edge, p, N, E, H, p, None)

    def bwd_dst(N, E, H, p=here, edge=here, ge=here, gdx=here):
        return lib.hscn_gatedgcn_bwd_dst(p, edge, edge, edge, p, p, p, edge, p, p, None, p, ge, gdx, N, E, H, p, None)

    def bwd_src(N, E, H, p=here, edge=here):
        return lib.hscn_gatedgcn_bwd_src(p, edge, edge, edge, edge, edge, p, p, N, E, H, p, None)

    for f in (fwd, bwd_dst, bwd_src):
        assert f(-1, 4, 16) == BADARG and f(4, -1, 16) == BADARG and f(4, 4, 0) == BADARG
        assert f(4, 4, 513) == UNSUPPORTED
        assert f(4, 4, 16, edge=None) == BADARG                       # NULL edge arrays with E > 0
        assert f(0, 0, 16, p=None, edge=None) == 0                    # nothing to do
    assert fwd(4, 4, 16, p=None) == BADARG and bwd_dst(4, 4, 16, p=None) == BADARG
    assert bwd_dst(4, 4, 16, ge=None) == BADARG and bwd_dst(4, 4, 16, gdx=None) == BADARG     # both or neither
    assert lib.hscn_gatedgcn_bwd_src(None, None, None, None, None, None, None, None, 4, 4, 16, None, None) == 0


# --------------------------------------------------------------------------- #
# 4. the restatement's identities and the backward formulas, float64
# --------------------------------------------------------------------------- #
def _case(N, E, H, seed, isolated=2):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N - isolated, (2, E), generator=g)
    t = [torch.randn(N, H, generator=g, dtype=torch.float64) for _ in range(4)]
    return t + [torch.randn(E, H, generator=g, dtype=torch.float64), ei]


def test_restatement_known_answer_and_identities():
    # one edge 0 -> 1 with e^ = 0: the gate is 1/2, h_1 = Ax_1 + (Bx_0 / 2) / (1/2 + 1e-6)
    one = torch.ones(2, 1, dtype=torch.float64)
    h, e = GG.aggregate(3 * one, 5 * one, one, -2 * one, one[:1], torch.tensor([[0], [1]]))
    assert float(e) == 0.0 and float(h[0]) == 3.0
    assert abs(float(h[1]) - (3.0 + 2.5 / (0.5 + 1e-6))) < 1e-15
    Ax, Bx, Dx, Ex, Ce, ei = _case(9, 30, 5, 0)
    h, e = GG.aggregate(Ax, Bx, Dx, Ex, Ce, ei)
    assert torch.equal(h[-2:], Ax[-2:])                                   # isolated nodes: h_i == Ax_i
    assert torch.equal(e, Dx[ei[1]] + Ex[ei[0]] + Ce)
    # a convex combination of the gathered Bx rows: Ax_i + min <= h_i <= Ax_i + max over the row's sources
    for i in range(7):
        rows = Bx[ei[0][ei[1] == i]]
        if rows.numel():
            assert bool(((h[i] - Ax[i]) <= rows.max(0).values + 1e-9).all() and ((h[i] - Ax[i]) >= rows.min(0).values - 1e-9).all())
    # permuting the edge list permutes the rows of e^ and leaves h unchanged up to the rounding of the summation order
    perm = torch.randperm(30, generator=torch.Generator().manual_seed(1))
    hp, ep = GG.aggregate(Ax, Bx, Dx, Ex, Ce[perm], ei[:, perm])
    assert torch.equal(ep, e[perm])
    assert float((hp - h).abs().max()) <= 30 * 2.0 ** -52 * float(h.abs().max())
    # skip leaves one edge out of both sums and keeps its row of e^
    k = 4
    keep = torch.arange(30) != k
    hs, es = GG.aggregate(Ax, Bx, Dx, Ex, Ce, ei, skip=k)
    hk, ek = GG.aggregate(Ax, Bx, Dx, Ex, Ce[keep], ei[:, keep])
    assert torch.equal(hs, hk) and torch.equal(es, e) and torch.equal(ek, e[keep])
    mags = GG.magnitudes(Ax, Bx, Dx, Ex, Ce, ei)
    _, den = GG.sums(Bx, e, ei)
    assert torch.equal(mags["den"], den) and torch.equal(mags["deg"].flatten(), torch.bincount(ei[1], minlength=9).double())
    assert bool((mags["num"] >= GG.sums(Bx, e, ei)[0].abs() - 1e-12).all())


@pytest.mark.parametrize("with_edge_cotangent", [True, False])
def test_hand_written_backward_matches_autograd(with_edge_cotangent):
    """The formulas of csrc/gatedgcn.hip's two backward passes (gn, gd, ge; the target- and the source-keyed sums)
    against torch.autograd on the restatement, in float64."""
    Ax, Bx, Dx, Ex, Ce, ei = _case(11, 40, 6, 3)
    ei[:, 0] = torch.tensor([2, 2])                                       # a loop and a repeated edge
    ei[:, 1] = ei[:, 2]
    g = torch.Generator().manual_seed(9)
    gh = torch.randn(11, 6, generator=g, dtype=torch.float64)
    ge = torch.randn(40, 6, generator=g, dtype=torch.float64) if with_edge_cotangent else None
    leaves = [t.clone().requires_grad_(True) for t in (Ax, Bx, Dx, Ex, Ce)]
    h, e = GG.aggregate(*leaves, ei)
    loss = (h * gh).sum() + ((e * ge).sum() if ge is not None else 0.0)
    loss.backward()
    hand = GG.backward_by_hand(Ax, Bx, Dx, Ex, Ce, ei, gh, ge)
    for name, leaf in zip(("Ax", "Bx", "Dx", "Ex", "Ce"), leaves):
        scale = float(leaf.grad.abs().max())
        assert float((hand[name] - leaf.grad).abs().max()) <= 1e-12 * max(scale, 1.0), name
    assert bool((hand["Bx"][-2:] == 0).all() and (hand["Dx"][-2:] == 0).all())      # isolated nodes


def test_model_restatements_run_and_carry_the_edge_state():
    torch.manual_seed(0)
    graphs = make_dataset("peptides_func", 3, seed=0, edge_features=True)
    b = Batch.from_data_list(graphs)
    x, ea = b.x.double(), b.edge_attr.double()
    m = GG.GatedGCNModelRef(9, 16, 10, 3, 3).double()
    seen = {}
    m.set_watch(lambda tag, t: seen.__setitem__(tag, t.shape))
    out = m(x, b.edge_index, ea, b.batch, 3)
    assert out.shape == (3, 10)
    assert seen == {f"layer {i} {k} output": s for i in range(2)
                    for k, s in (("node", (b.num_nodes, 16)), ("edge", (b.edge_index.size(1), 16)))}
    out.sum().backward()
    # the last layer's edge output is dropped: its C, D and E still act through the gates
    assert all(p.grad is not None for p in m.parameters())
    assert m(x, b.edge_index, ea, b.batch, 3, skip=5).sub(out).abs().max() > 0
    g = GG.GatedGPSRef(9, 16, 10, 2, 4, edge_dim=3).double()
    ptr = torch.tensor([0] + list(torch.cumsum(torch.tensor([gr.num_nodes for gr in graphs]), 0)))
    pred = g(x, b.edge_index, ea, b.batch, ptr, 3)
    assert pred.shape == (3, 10)
    pred.sum().backward()
    assert g.edge_encoder.weight.grad is not None and float(g.edge_encoder.weight.grad.abs().max()) > 0
    # the last GPS layer's edge output is dropped: its bn_edge_e sees no cotangent
    assert g.layers[1].conv.bn_edge_e.weight.grad is None and g.layers[0].conv.bn_edge_e.weight.grad is not None
