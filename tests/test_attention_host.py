"""Global attention, everything that answers without a GPU: the C ABI's exports, envelope and argument checks (all
before any launch), ``GPSConfig``, every refusal of the Python layers by its message, the parameter interchange of
``MultiheadSelfAttention`` with ``torch.nn.MultiheadAttention``, and the resident entry points refusing ``GPS``."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, GPSConfig
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS, build_gps
from graph_hscn.nn import functional as Fh
from graph_hscn.nn.attention import MultiheadSelfAttention
from graph_hscn.nn.gps import GPSLayer

BADARG, UNSUPPORTED = -1, -3
_BUF = ctypes.create_string_buffer(512)
_HERE = (ctypes.addressof(_BUF) + 15) & ~15          # a 16-byte aligned host address standing in for a pointer


def test_exports_and_envelope_edges():
    lib = _hip.lib()
    for name in ("hscn_attention_supported", "hscn_attention_tile", "hscn_attention_chunk", "hscn_attention_fwd",
                 "hscn_attention_bwd_q", "hscn_attention_bwd_kv"):
        assert hasattr(lib, name) and name in _hip.exported_symbols()
    assert lib.hscn_attention_tile() >= 1 and lib.hscn_attention_chunk() >= 1
    # dh: 0 and 2 (below 4), 4 and 64 (the edges), 68 (above), 6 (not a multiple of 4)
    for dh, ok in ((0, 0), (2, 0), (4, 1), (6, 0), (64, 1), (68, 0), (-4, 0)):
        assert lib.hscn_attention_supported(1, dh) == ok, dh
    # heads * dh: 512 is in, 516 is out, however it is split
    assert lib.hscn_attention_supported(8, 64) == 1 and lib.hscn_attention_supported(128, 4) == 1
    assert lib.hscn_attention_supported(129, 4) == 0 and lib.hscn_attention_supported(43, 12) == 0     # 516
    assert lib.hscn_attention_supported(0, 16) == 0 and lib.hscn_attention_supported(-1, 16) == 0
    assert Fh.attention_supported(4, 24) and not Fh.attention_supported(4, 2)
    assert (Fh.ATTN_MIN_HEAD_DIM, Fh.ATTN_MAX_HEAD_DIM, Fh.ATTN_MAX_WIDTH) == (4, 64, 512)


def _fwd(qkv, ptr, N, B, max_nodes, heads, dh, out, lse, flag):
    return _hip.lib().hscn_attention_fwd(qkv, ptr, N, B, max_nodes, heads, dh, out, lse, flag, None)


def _bwd_q(p, N, B, max_nodes, heads, dh):
    return _hip.lib().hscn_attention_bwd_q(p, p, p, p, p, N, B, max_nodes, heads, dh, p, p, p, None)


def _bwd_kv(p, N, B, max_nodes, heads, dh):
    return _hip.lib().hscn_attention_bwd_kv(p, p, p, p, p, N, B, max_nodes, heads, dh, p, p, None)


def test_argument_checks_answer_before_any_launch():
    H = _HERE
    # negative sizes
    assert _fwd(H, H, -1, 1, 4, 1, 4, H, H, H) == BADARG
    assert _fwd(H, H, 4, -1, 4, 1, 4, H, H, H) == BADARG
    assert _fwd(H, H, 4, 1, -1, 1, 4, H, H, H) == BADARG
    assert _fwd(H, H, 1 << 31, 1, 4, 1, 4, H, H, H) == BADARG
    # the envelope
    for heads, dh in ((1, 0), (1, 2), (1, 68), (129, 4), (0, 8), (2, 6)):
        assert _fwd(H, H, 4, 1, 4, heads, dh, H, H, H) == UNSUPPORTED, (heads, dh)
        assert _bwd_q(H, 4, 1, 4, heads, dh) == UNSUPPORTED
        assert _bwd_kv(H, 4, 1, 4, heads, dh) == UNSUPPORTED
    # nothing to do: no pointer is looked at
    assert _fwd(None, None, 0, 3, 4, 1, 4, None, None, None) == 0
    assert _fwd(None, None, 5, 0, 4, 1, 4, None, None, None) == 0
    assert _bwd_q(None, 0, 0, 0, 2, 8) == 0 and _bwd_kv(None, 0, 0, 0, 2, 8) == 0
    # null pointers, one at a time
    for k in range(5):
        args = [H] * 5
        args[k] = None
        assert _fwd(args[0], args[1], 4, 1, 4, 1, 4, args[2], args[3], args[4]) == BADARG, k
    assert _bwd_q(None, 4, 1, 4, 1, 4) == BADARG and _bwd_kv(None, 4, 1, 4, 1, 4) == BADARG
    # rows are read 16 bytes at a time
    assert _fwd(H + 4, H, 4, 1, 4, 1, 4, H, H, H) == BADARG
    assert _fwd(H, H, 4, 1, 4, 1, 4, H + 8, H, H) == BADARG


def test_gps_config_validation():
    cfg = GPSConfig("relu")
    assert (cfg.local_conv_type, cfg.num_heads, cfg.norm, cfg.task_level) == ("gine", 4, "layer", "graph")
    assert cfg.hidden_channels == 16 and cfg.num_layers == 3
    GPSConfig("relu", None, 64, 2, 8, 0.1, "batch", "node")
    GPSConfig("relu", "GCN", 512, 1, 8, 0.0, None, "link")
    with pytest.raises(ValueError, match="divisible by num_heads"):
        GPSConfig("relu", hidden_channels=18, num_heads=4)
    with pytest.raises(ValueError, match="head width 2"):
        GPSConfig("relu", hidden_channels=8, num_heads=4)
    with pytest.raises(ValueError, match="head width 68"):
        GPSConfig("relu", hidden_channels=68, num_heads=1)
    with pytest.raises(ValueError, match="at most 512"):
        GPSConfig("relu", hidden_channels=516, num_heads=43)
    with pytest.raises(ValueError, match="norm must be"):
        GPSConfig("relu", norm="instance")
    with pytest.raises(ValueError, match="local_conv_type"):
        GPSConfig("relu", local_conv_type="transformer")
    with pytest.raises(ValueError, match="task_level"):
        GPSConfig("relu", task_level="edge")
    with pytest.raises(ValueError, match="positive"):
        GPSConfig("relu", num_heads=0)
    with pytest.raises(ValueError, match=r"\[0.0, 1.0\)"):
        GPSConfig("relu", dropout=1.5)
    m = build_gps(GPSConfig("relu", None, 16, 2, 4, 0.0), 9, 10)
    assert isinstance(m, GPS) and len(m.layers) == 2 and m.layers[0].conv is None and m.head_width() == 10


def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match="dropout on the attention weights"):
        MultiheadSelfAttention(16, 4, dropout=0.1)
    with pytest.raises(ValueError, match="divisible by num_heads"):
        MultiheadSelfAttention(18, 4)
    with pytest.raises(ValueError, match=r"multiple of 4 in \[4, 64\].*embed_dim <= 512"):
        MultiheadSelfAttention(8, 4)                       # head width 2
    with pytest.raises(ValueError, match="envelope"):
        MultiheadSelfAttention(136, 2)                     # head width 68
    with pytest.raises(ValueError, match="envelope"):
        MultiheadSelfAttention(516, 43)                    # head width 12, 516 columns
    att = MultiheadSelfAttention(16, 4)
    x = torch.randn(5, 16)
    ptr32 = torch.tensor([0, 5], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="need_weights"):
        att(x, ptr32=ptr32, max_nodes=5, need_weights=True)
    for name in ("attn_mask", "key_padding_mask", "attn_bias"):
        with pytest.raises(NotImplementedError, match=name):
            att(x, ptr32=ptr32, max_nodes=5, **{name: torch.zeros(5, 5)})
    with pytest.raises(ValueError, match="graph boundaries"):
        att(x)
    with pytest.raises(ValueError, match="carries no ptr32"):
        att(x, SimpleNamespace(max_nodes=5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att(x, ptr32=ptr32, max_nodes=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fh.SelfAttentionFn.apply(torch.randn(5, 48), ptr32, 5, 4)
    with pytest.raises(ValueError, match="envelope"):
        Fh.SelfAttentionFn.apply(torch.randn(5, 24), ptr32, 5, 4)       # head width 2
    with pytest.raises(TypeError, match="int32"):
        Fh.SelfAttentionFn.apply(torch.randn(5, 48), ptr32.long(), 5, 4)
    with pytest.raises(ValueError, match="local_conv must be"):
        GPSLayer(16, "gin", 4)
    with pytest.raises(ValueError, match="norm must be"):
        GPSLayer(16, None, 4, norm="instance")
    with pytest.raises(ValueError, match="task_level"):
        GPS(9, 16, 10, 2, task_level="edge")
    # gine without edge features, as MPNN._edge_attr words it
    graphs = make_dataset("peptides_func", 2, seed=0)
    from graph_hscn.data import Batch
    m = GPS(9, 16, 10, 1, 4, "gine")
    with pytest.raises(ValueError, match="carries no\\s+edge_attr"):
        m(Batch.from_data_list(graphs))


@pytest.mark.parametrize("D,heads,bias", [(16, 4, True), (96, 4, True), (64, 1, False)])
def test_parameters_interchange_with_torch_multihead_attention(D, heads, bias):
    torch.manual_seed(0)
    ours = MultiheadSelfAttention(D, heads, bias=bias)
    theirs = torch.nn.MultiheadAttention(D, heads, bias=bias, batch_first=True)
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b)
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    assert [n for n, _ in ours.named_parameters()] == [n for n, _ in theirs.named_parameters()]
    ours.load_state_dict(b, strict=True)
    for k in b:
        assert torch.equal(ours.state_dict()[k], b[k])
    ours.reset_parameters()
    theirs.load_state_dict(ours.state_dict(), strict=True)
    for k, v in ours.state_dict().items():
        assert torch.equal(theirs.state_dict()[k], v)
    # the same initialisation scheme: identical draws from the same generator state
    torch.manual_seed(7)
    p = MultiheadSelfAttention(D, heads, bias=bias).state_dict()
    torch.manual_seed(7)
    t = torch.nn.MultiheadAttention(D, heads, bias=bias).state_dict()
    assert torch.equal(p["in_proj_weight"], t["in_proj_weight"])
    assert torch.equal(p["out_proj.weight"], t["out_proj.weight"])
    if bias:
        assert not p["in_proj_bias"].any() and not p["out_proj.bias"].any()
    bound = 1.0 / D ** 0.5                                  # kaiming_uniform(a = sqrt 5) on [D, D]
    assert float(p["out_proj.weight"].abs().max()) <= bound


@pytest.mark.parametrize("task_level", ["graph", "node", "link"])
def test_resident_entry_points_refuse_gps_before_anything_is_launched(task_level):
    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    m = GPS(9, 16, 10, 2, 4, "gcn", ACT_DICT["relu"], task_level=task_level)      # on the CPU: nothing can launch
    reason = m.resident_reason()
    assert "global attention" in reason and m.resident_reason(batch=object()) == reason
    assert m.engine == "layered" and not m.supported() and m.layered_only
    graphs = make_dataset("peptides_func", 4, seed=0)
    m.engine = "resident"
    with pytest.raises(RuntimeError, match="global attention"):
        m(None)
    m.engine = "nonsense"
    with pytest.raises(ValueError, match="engine must be"):
        m(None)
    m.engine = "layered"
    with pytest.raises(RuntimeError, match="global attention"):
        MPNNResidentTrainStep(m, None, "cross_entropy")
    with pytest.raises(RuntimeError, match="global attention"):
        batching.resident_step(m, None, "cross_entropy")           # what replay.CapturedStep builds its step with
    with pytest.raises(RuntimeError, match="global attention"):
        DeviceEvaluator(graphs, m, "cross_entropy", 4)
    cfg = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    with pytest.raises(RuntimeError, match="global attention"):
        fit_resident(None, opt, cfg, graphs, [], m, 4)
    assert batching.score_width(m, torch.zeros(3, dtype=torch.int64)) == 10


def test_linear_wide_chunks_by_the_library_limit(monkeypatch):
    """``linear_wide`` cuts the output columns so that every chunk's weight fits ``hscn_linear_fwd``'s LDS image; the
    Python constant and the library's limit are pinned to each other through the library's own answer."""
    lib = _hip.lib()
    H = _HERE
    limit = Fh.LINEAR_MAX_WEIGHT_BYTES
    assert limit == 160 * 1024
    # one weight row more than the limit allows at I = 512: refused before any launch (a call at the limit would launch)
    over = limit // (4 * 512) + 1
    assert lib.hscn_linear_fwd(H, H, None, None, None, None, None, H, 1, 512, over, 0, 0, None) == UNSUPPORTED
    shapes = []

    def cpu_linear(x, W, bias=None, act="identity"):
        shapes.append(tuple(W.shape))
        y = x @ W.t() + (0 if bias is None else bias)
        return torch.relu(y) if act == "relu" else y

    monkeypatch.setattr(Fh, "linear", cpu_linear)
    g = torch.Generator().manual_seed(0)
    for I, O, act in ((512, 1536, "identity"), (512, 1024, "relu"), (1024, 512, "identity"), (16, 48, "identity")):
        shapes.clear()
        x, W, b = torch.randn(5, I, generator=g), torch.randn(O, I, generator=g), torch.randn(O, generator=g)
        y = Fh.linear_wide(x, W, b, act)
        # the same sums of I + 1 terms in another blocking: within the a-priori float32 bound of each other
        lim = 2 * 3.0 * (I + 2) * 2.0 ** -24 * float((x.abs() @ W.abs().t() + b.abs()).max())
        assert float((y - cpu_linear(x, W, b, act)).abs().max()) <= lim
        chunks = shapes[:-1]
        assert sum(o for o, _ in chunks) == O and all(i == I and i * o * 4 <= limit for o, i in chunks)
        assert (len(chunks) == 1) == (I * O * 4 <= limit)
    with pytest.raises(ValueError, match="beyond the kernel's envelope"):
        Fh.linear_wide(torch.randn(2, 20000), torch.randn(8, 20000))
