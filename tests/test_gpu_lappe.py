"""The fused LapPE DeepSet operator (csrc/lappe.hip, nn.functional.LapPEDeepSetFn) against the float64 oracle of
tests/lappe_oracle.py, through ``helpers.f64_close`` with the project's c = 3:

  * ``pe_sum``: n = sum_l (fan_in_l + 1 + 4) + K, mag = the chain on absolute values summed over the valid frequencies;
  * a parameter gradient: n + the number of valid (node, frequency) samples, mag = the same backward over absolute
    values (the true evaluation's ReLU gates);
  * the tooth of each bound in the same test: the oracle with frequency 0 left out must be rejected.

A gradient is discontinuous where a pre-activation crosses zero, so the inputs are conditioned on the REFERENCE (the
idea of ``helpers.KinkGuard``): a case takes the first seed whose float64 evaluation keeps every pre-activation of a
valid sample at least 4e-6 from zero (64 float32 ulps of a value of size 1; a float32 chain of these lengths lands
within a few ulps) and whose gradients all feel frequency 0.  The guard only removes false alarms: a flipped gate
fails the bound, it cannot make it pass.

Shapes: N in {1, T-1, T, T+1, 2T+3} with T = hscn_lappe_tile(); rows with 1, 2, ... valid frequencies and one all-NaN
row (``lappe_oracle.make_inputs``); K in {1, 4, 10, 64}, dim_pe in {4, 16, 32}, layers in {1, 2, 3, 4} as a covering
subset."""
import functools

import pytest
import torch

from graph_hscn import _hip
from graph_hscn.nn import functional as Fh
from tests import lappe_oracle as LO
from tests.helpers import f64_close

DEV = "cuda"
T = int(_hip.lib().hscn_lappe_tile())
SEED = 0xC0FFEE12345
# (layers, dim_pe, K, N)
CASES = [(1, 4, 1, 1), (2, 16, 10, T - 1), (2, 16, 10, T), (3, 32, 4, T + 1), (2, 4, 4, 2 * T + 3), (4, 4, 64, 1),
         (1, 32, 64, 3), (3, 16, 1, T), (4, 32, 10, 70)]
MARGIN = 4e-6


class _Spy:
    """Names of the C-ABI entries issued through nn.functional while active (tests/test_gpu_attention.py's)."""

    def __init__(self, monkeypatch):
        self.names = []
        real = Fh.call

        def call(name, *a):
            self.names.append(name)
            return real(name, *a)

        monkeypatch.setattr(Fh, "call", call)


@functools.lru_cache(maxsize=None)
def _case(layers, dim_pe, K, N, flip):
    """Inputs and every float64 reference of a case, computed once and left unchanged."""
    sg = LO.signs(K, SEED) if flip else None
    for seed in range(32):
        vec, val, Ws, bs, g = LO.make_inputs(N, K, dim_pe, layers, seed=1000 * layers + 10 * K + seed)
        ref, gref, margin = LO.chain(vec, val, Ws, bs, sg, g=g)
        drop, gdrop, _ = LO.chain(vec, val, Ws, bs, sg, g=g, drop_freq=0)
        if margin >= MARGIN and all(float((a - b).abs().max()) > 0 for a, b in zip(gref, gdrop)):
            break
    else:
        raise AssertionError("no seed keeps the reference's pre-activations away from zero")
    mag, gmag, _ = LO.chain(vec, val, Ws, bs, sg, g=g, absolute=True)
    samples = int((~torch.isnan(vec)).sum())
    return dict(vec=vec, val=val, Ws=Ws, bs=bs, g=g, ref=ref, gref=gref, drop=drop, gdrop=gdrop, mag=mag, gmag=gmag,
                samples=samples, sg=sg)


def _run(c, seed):
    leaves = [t.to(DEV).requires_grad_(True) for wb in zip(c["Ws"], c["bs"]) for t in wb]
    out = Fh.LapPEDeepSetFn.apply(c["vec"].to(DEV), c["val"].to(DEV), leaves[0::2], leaves[1::2], seed)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("layers,dim_pe,K,N", CASES)
def test_forward_and_parameter_gradients_within_the_float64_bound(layers, dim_pe, K, N, flip, monkeypatch):
    c = _case(layers, dim_pe, K, N, flip)
    what = f"lappe L={layers} dim_pe={dim_pe} K={K} N={N} flip={flip}"
    spy = _Spy(monkeypatch)
    out, grads = _run(c, SEED if flip else None)
    assert spy.names == ["hscn_lappe_fwd", "hscn_lappe_bwd"]
    n = LO.bound_n(dim_pe, layers, K)
    assert out.shape == (N, dim_pe)
    assert f64_close(out, c["ref"], c["mag"], n, what=what + " pe_sum"), what
    assert not f64_close(out, c["drop"], c["mag"], n), f"{what}: the bound cannot see a dropped frequency"
    if N >= 3:
        assert float(out[1].abs().max()) == 0.0                 # the all-NaN row
    if flip and bool((c["sg"] < 0).any()):                     # the signs matter: the unflipped oracle is rejected
        plain, _, _ = LO.chain(c["vec"], c["val"], c["Ws"], c["bs"], None)
        assert not f64_close(out, plain, c["mag"], n), f"{what}: the bound cannot see the sign flips"
    names = [f"{p}_{l}" for l in range(layers) for p in ("gW", "gb")]
    for name, got, ref, drop, mag in zip(names, grads, c["gref"], c["gdrop"], c["gmag"]):
        assert got is not None and got.shape == ref.shape, name
        assert f64_close(got, ref, mag, n + c["samples"], what=f"{what} {name}"), f"{what} {name}"
        assert not f64_close(got, drop, mag, n + c["samples"]), f"{what} {name}: the bound cannot see a dropped frequency"


@pytest.mark.gpu
def test_the_backward_uses_the_forward_s_signs():
    """Gradients under a pinned seed are the oracle's under the Philox signs and are rejected by the oracle under the
    signs of another seed (the forward alone would not show a backward that regenerates other signs)."""
    layers, dim_pe, K, N = 2, 16, 10, T
    c = _case(layers, dim_pe, K, N, True)
    _, grads = _run(c, SEED)
    other = LO.signs(K, SEED + 1)
    assert not torch.equal(other, c["sg"])
    _, gother, _ = LO.chain(c["vec"], c["val"], c["Ws"], c["bs"], other, g=c["g"])
    n = LO.bound_n(dim_pe, layers, K) + c["samples"]
    assert f64_close(grads[0], c["gref"][0], c["gmag"][0], n)
    assert not f64_close(grads[0], gother[0], c["gmag"][0], n)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits():
    for case in [(2, 16, 10, 2 * T + 3), (4, 32, 4, T + 1)]:
        vec, val, Ws, bs, g = LO.make_inputs(case[3], case[2], case[1], case[0], seed=9)
        c = dict(vec=vec, val=val, Ws=Ws, bs=bs, g=g)
        o1, g1 = _run(c, SEED)
        o2, g2 = _run(c, SEED)
        assert torch.equal(o1, o2)
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("layers,dim_pe,K", [(2, 16, 10), (4, 32, 64), (1, 4, 1)])
def test_a_row_is_bitwise_the_same_alone_and_inside_a_larger_batch(layers, dim_pe, K):
    N = 2 * T + 3
    vec, val, Ws, bs, _ = LO.make_inputs(N, K, dim_pe, layers, seed=21)
    Wd, bd = [w.to(DEV) for w in Ws], [b.to(DEV) for b in bs]
    full = Fh.LapPEDeepSetFn.apply(vec.to(DEV), val.to(DEV), Wd, bd, SEED)
    for i in (0, 2, T - 1, T, T + 5, N - 1):
        alone = Fh.LapPEDeepSetFn.apply(vec[i:i + 1].to(DEV), val[i:i + 1].to(DEV), Wd, bd, SEED)
        assert torch.equal(alone[0], full[i]), i
    part = Fh.LapPEDeepSetFn.apply(vec[T - 3:T + 9].contiguous().to(DEV), val[T - 3:T + 9].contiguous().to(DEV), Wd, bd, SEED)
    assert torch.equal(part, full[T - 3:T + 9])


@pytest.mark.gpu
def test_no_nodes_launch_nothing(monkeypatch):
    _, _, Ws, bs, _ = LO.make_inputs(1, 10, 16, 2, seed=0)
    leaves = [t.to(DEV).requires_grad_(True) for wb in zip(Ws, bs) for t in wb]
    spy = _Spy(monkeypatch)
    empty = torch.empty(0, 10, device=DEV)
    out = Fh.LapPEDeepSetFn.apply(empty, empty.clone(), leaves[0::2], leaves[1::2], 5)
    assert out.shape == (0, 16)
    out.sum().backward()
    assert spy.names == []
    for t in leaves:
        assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().max()) == 0.0


@pytest.mark.gpu
def test_statistics_that_require_grad_are_refused_by_name():
    vec, val, Ws, bs, _ = LO.make_inputs(3, 4, 4, 1, 0)
    Wd, bd = [w.to(DEV) for w in Ws], [b.to(DEV) for b in bs]
    with pytest.raises(ValueError, match="vec requires grad"):
        Fh.LapPEDeepSetFn.apply(vec.to(DEV).requires_grad_(True), val.to(DEV), Wd, bd, None)
    with pytest.raises(ValueError, match="val requires grad"):
        Fh.LapPEDeepSetFn.apply(vec.to(DEV), val.to(DEV).requires_grad_(True), Wd, bd, None)


def _encoder(layers, post, **kw):
    from graph_hscn.config.config import LapPEConfig
    from graph_hscn.encoder import LapPENodeEncoder
    torch.manual_seed(3)
    cfg = LapPEConfig(dim_in=9, dim_emb=32, dim_pe=8, layers=layers, post_layers=post, eigen_max_freqs=10, **kw)
    return LapPENodeEncoder(cfg, 9, 32).to(DEV)


@pytest.mark.gpu
def test_encoder_flips_in_training_mode_only(monkeypatch):
    enc = _encoder(2, 0)
    vec, val, _, _, _ = LO.make_inputs(T + 1, 10, 8, 2, seed=4)
    chain = [enc.linear_A] + list(enc.pe_encoder)
    Ws, bs = [m.weight for m in chain], [m.bias for m in chain]
    n = LO.bound_n(8, 2, 10)
    sg = LO.signs(10, 11)
    assert bool((sg < 0).any())
    plain, _, _ = LO.chain(vec, val, Ws, bs, None)
    flipped, _, _ = LO.chain(vec, val, Ws, bs, sg)
    mag, _, _ = LO.chain(vec, val, Ws, bs, None, absolute=True)
    enc.pe_seed = 11
    enc.train()
    spy = _Spy(monkeypatch)
    got = enc.pe(vec.to(DEV), val.to(DEV).unsqueeze(2))
    got.sum().backward()
    assert spy.names == ["hscn_lappe_fwd", "hscn_lappe_bwd"]
    assert f64_close(got, flipped, mag, n) and not f64_close(got, plain, mag, n)
    enc.eval()
    got = enc.pe(vec.to(DEV), val.to(DEV))
    assert f64_close(got, plain, mag, n) and not f64_close(got, flipped, mag, n)
    enc.train()
    enc.sign_flip = False                          # cfg.sign_flip = False: training mode leaves the signs too
    assert torch.equal(enc.pe(vec.to(DEV), val.to(DEV)), got)
    enc.sign_flip, enc.pe_seed = True, None        # unpinned: a fresh host seed per call
    a, b = enc.pe(vec.to(DEV), val.to(DEV)), enc.pe(vec.to(DEV), val.to(DEV))
    assert a.shape == b.shape == (T + 1, 8)


@pytest.mark.gpu
def test_post_mlp_adds_linear_calls_and_nothing_else(monkeypatch):
    enc = _encoder(3, 2)
    vec, val, _, _, _ = LO.make_inputs(70, 10, 8, 3, seed=4)
    enc.eval()
    spy = _Spy(monkeypatch)
    pe = enc.pe(vec.to(DEV), val.to(DEV))
    assert spy.names == ["hscn_lappe_fwd", "hscn_linear_fwd", "hscn_linear_fwd"]
    pe.sum().backward()
    rest = spy.names[3:]
    assert rest[-1] == "hscn_lappe_bwd" and rest.count("hscn_lappe_bwd") == 1 and "hscn_lappe_fwd" not in rest
    assert set(rest[:-1]) <= {"hscn_linear_fwd", "hscn_linear_bwd_w", "hscn_act_bwd"}
    # [x | pe] through forward(), on the oracle's values
    from graph_hscn.data import Batch, Data
    b = Batch.from_data_list([Data(x=torch.randn(70, 9), edge_index=torch.zeros(2, 0, dtype=torch.long))]).to(DEV)
    b.eigvecs_sn, b.eigvals_sn = vec.to(DEV), val.to(DEV).unsqueeze(2)
    x = b.x.clone()
    out = enc(b).x
    assert out.shape == (70, 32)
    assert torch.equal(out[:, 24:], pe.detach())
    assert torch.equal(out[:, :24], enc.linear_x(x).detach())
    for m in list(enc.post_mlp) + [enc.linear_A] + list(enc.pe_encoder):
        assert m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all())
