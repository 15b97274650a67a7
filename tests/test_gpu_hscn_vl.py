"""HSCN with the opt-in ("virtual", "to", "local") relation: the one-launch training step, the forward-only launch,
the layered autograd path and the device loops, against a CPU reference composed from oracle.models.HSCN (one more
P.GATConv per layer under ``virtual__to__local``, the lv edge list flipped and appended to ``edge_index_dict``).

Comparison rule: this project's f64 referee (tests/test_gpu_mpnn_resident.py: _refereed, k = 2, ulps = 8, copied):
    |HIP - f64|  <=  2 |oracle_f32 - f64| + 8 ulp(scale),      ulp(scale) = 2^-23 max|f64|
For lv's att_src / att_dst the float64 gradient can be a cancellation residue (within a cluster
sum_i alpha_i (d_i - sum alpha d) = 0: where every score of the row has one sign the leaky ReLU does not break the tie),
so their ulp term is scaled by the same gradient evaluated on absolute values where that is larger
(tests/test_gpu_gat_self_loops.py: attention_grad_abs_sums does the same)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import models as OM
from oracle import pyg_ops as P
from tests.helpers import DEV, grads_close, hetero_batch

pytestmark = pytest.mark.gpu

LL, VV, LV, VL = OM.LL, OM.VV, OM.LV, ("virtual", "to", "local")


def _refereed(hip, o32, o64, what, k=2.0, ulps=8.0, mag=None):
    hip, o32, o64 = (t.detach().cpu().double() for t in (hip, o32, o64))
    e_hip = float((hip - o64).abs().max())
    e_o32 = float((o32 - o64).abs().max())
    scale = float(o64.abs().max())
    if mag is not None:
        scale = max(scale, float(mag.detach().abs().max()))
    ulp = 2.0 ** -23 * scale
    ok = e_hip <= k * e_o32 + ulps * ulp
    print(f"[f64 referee] {what}: |HIP-f64|={e_hip:.3e} |oracle32-f64|={e_o32:.3e} ulp(scale)={ulp:.3e}"
          + ("" if ok else "  <-- FAIL"))
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# models and batches
# ---------------------------------------------------------------------------------------------------------------------
def _models(F, H, C, L, act, seed):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(seed)
    om = OM.HSCN("GAT", "GCN", "GCN", OM.ACT[act], F, H, C, L)
    for l, conv in enumerate(om.convs):
        fin = F if l == 0 else H
        conv.convs["virtual__to__local"] = P.GATConv((fin, fin), H)
    with torch.no_grad():
        for n_, q in om.named_parameters():
            if n_.endswith("bias"):
                q.normal_(0, 0.1)
    pm = HSCN("GAT", "GCN", "GCN", ACT_DICT[act], F, H, C, L, vl_conv="GAT").to(DEV)
    assert sorted(pm.state_dict()) == sorted(om.state_dict())
    pm.load_state_dict(om.state_dict())
    return om, pm


def _hetero(graphs, ids, K):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    return [hetero_from_clusters(g, i, K) for g, i in zip(graphs, ids)]


def _collate(hs):
    from graph_hscn.data import HeteroBatch
    return HeteroBatch.from_data_list(hs)


def _hand_graphs(loss_fn, C=10, F=9):
    """Five graphs, K = 4: (1) one node, one cluster, no ll edge; (2) 7 nodes: an isolated node, an ll self loop, a
    repeated edge; (3) 70 nodes in 2 clusters, one of them a single member; (4) 150 nodes in 2 clusters (a member list
    longer than a wave); (5) 20 nodes, all 4 clusters non-empty.  Features from N(0, 1)."""
    from graph_hscn.data import Data
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(5)

    def y():
        return (torch.rand(1, C, generator=g) < .5).float() if loss_fn == "cross_entropy" else torch.randn(1, C, generator=g)

    def sym(n, e):
        ei = torch.randint(0, n, (2, e), generator=g)
        ei = ei[:, ei[0] != ei[1]]
        return torch.cat([ei, ei.flip(0)], 1)

    graphs, ids = [], []
    graphs.append(Data(x=torch.randn(1, F, generator=g), edge_index=torch.zeros(2, 0, dtype=torch.long), y=y()))
    ids.append(np.array([2]))
    ei = torch.tensor([[0, 1, 1, 2, 3, 3, 4, 1, 5], [1, 0, 2, 1, 3, 4, 3, 2, 4]])      # node 6 isolated; 3->3; 1->2 twice
    graphs.append(Data(x=torch.randn(7, F, generator=g), edge_index=ei, y=y()))
    ids.append(np.array([0, 0, 1, 1, 3, 3, 0]))
    graphs.append(Data(x=torch.randn(70, F, generator=g), edge_index=sym(70, 80), y=y()))
    i3 = np.ones(70, dtype=np.int64)
    i3[17] = 3
    ids.append(i3)
    graphs.append(Data(x=torch.randn(150, F, generator=g), edge_index=sym(150, 170), y=y()))
    i4 = rng.integers(0, 2, 150) * 2
    i4[:70] = 0                                             # >= 70 members in one cluster
    ids.append(i4)
    graphs.append(Data(x=torch.randn(20, F, generator=g), edge_index=sym(20, 25), y=y()))
    i5 = rng.integers(0, 4, 20)
    i5[:4] = np.arange(4)
    ids.append(i5)
    return _hetero(graphs, ids, 4)


def _peptides(B, K, seed, F=9, max_nodes=None, draw=4):
    """``tests.helpers.hetero_batch``'s graphs and cluster draw (rng(seed).integers(0, K, n) per graph), features
    replaced by N(0, 1) draws of width F (the attention scores then straddle zero)."""
    _, graphs = hetero_batch("peptides_func", B * draw if max_nodes else B, K, seed)
    rng = np.random.default_rng(seed)
    ids = [rng.integers(0, K, g.num_nodes) for g in graphs]
    if max_nodes:
        keep = [i for i, g in enumerate(graphs) if g.num_nodes <= max_nodes][:B]
        assert len(keep) == B
        graphs, ids = [graphs[i] for i in keep], [ids[i] for i in keep]
    gen = torch.Generator().manual_seed(seed)
    for g in graphs:
        g.x = torch.randn(g.num_nodes, F, generator=gen)
    return _hetero(graphs, ids, K)


def _ref_inputs(hb, dtype):
    eid = {k: v for k, v in hb.edge_index_dict.items()}
    eid[VL] = eid[LV].flip(0)
    return {k: v.to(dtype) for k, v in hb.x_dict.items()}, eid


def _oracle(om, hb, loss_fn, dtype):
    """pred / loss / score / every parameter gradient (None where autograd leaves none) and, per live lv convolution,
    the att_src / att_dst gradients evaluated on absolute values."""
    m = copy.deepcopy(om).to(dtype)
    m.zero_grad(set_to_none=True)
    kept = {}

    def hook(name):
        def fn(mod, inp, out):
            out.retain_grad()
            kept[name] = (mod, inp[0][0].detach(), inp[0][1].detach(), inp[1], out)
        return fn

    hs = [conv.convs["local__to__virtual"].register_forward_hook(hook(f"convs.{l}.convs.local__to__virtual"))
          for l, conv in enumerate(m.convs)]
    x_dict, eid = _ref_inputs(hb, dtype)
    pred = m(x_dict, eid, hb["local"].batch, hb.num_graphs)
    y = hb["local"].y.to(dtype)
    loss = TF.binary_cross_entropy_with_logits(pred, y) if loss_fn == "cross_entropy" else TF.l1_loss(pred, y)
    loss.backward()
    for h in hs:
        h.remove()
    out = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "score": torch.sigmoid(pred.detach())}
    for n_, q in m.named_parameters():
        out[n_] = q.grad
    mags = {}
    with torch.no_grad():
        for name, (c, xs, xd, ei, o) in kept.items():
            if o.grad is None:
                continue
            h_s, h_d = c.lin_src(xs), c.lin_dst(xd)
            a_s, a_d = (h_s * c.att_src.view(-1)).sum(-1), (h_d * c.att_dst.view(-1)).sum(-1)
            row, col = ei[0], ei[1]
            pre = a_s[row] + a_d[col]
            alpha = P.segment_softmax(torch.where(pre > 0, pre, pre * c.negative_slope), col, xd.size(0))
            d = (o.grad[col] * h_s[row]).sum(-1)
            ts = torch.zeros(xd.size(0), dtype=dtype).index_add(0, col, alpha * d)
            gp = (alpha * (d - ts[col]) * torch.where(pre > 0, 1.0, c.negative_slope)).abs()
            mags[name + ".att_src"] = (gp.view(-1, 1) * h_s[row].abs()).sum(0)
            mags[name + ".att_dst"] = (gp.view(-1, 1) * h_d[col].abs()).sum(0)
    return out, mags


DEAD = ("convs.{l}.convs.local__to__virtual.", "convs.{l}.convs.virtual__to__virtual.")
VL_ZERO = ("lin_dst.weight", "att_src", "att_dst")


def _check_all(got, o32, o64, mags, L, tag):
    """``got``: name -> tensor (a name autograd leaves without a gradient must be absent)."""
    bad = []
    for k, ref in o64.items():
        if ref is None:
            assert any(k.startswith(d.format(l=L - 1)) for d in DEAD), k        # only the last layer's lv / vv
            assert k not in got or got[k] is None, f"{tag}: {k} has a gradient, autograd gives none"
            continue
        assert k in got and got[k] is not None, f"{tag}: {k} is missing"
        if not _refereed(got[k], o32[k], ref, f"{tag} {k}", mag=mags.get(k)):
            bad.append(k)
        if "virtual__to__local" in k and k.endswith(VL_ZERO):
            assert float(ref.abs().max()) == 0.0                                # float64 autograd: exactly zero
            assert bool((got[k] == 0).all()), f"{tag}: {k} must be exactly zero"
    assert not bad, (tag, bad)


def _step_outputs(step, pm):
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    out = {"pred": step.pred, "loss": step.loss.reshape(1), "score": step.score}
    for q, g in step.param_grads:
        out[names[id(q)]] = g
    return out


def _run_step(pm, hbd, loss_fn, **kw):
    from graph_hscn.step import VLResidentTrainStep
    step = VLResidentTrainStep(pm, hbd, loss_fn, **kw)
    step.run()
    torch.cuda.synchronize()
    step.check()
    return step


def _references(om, hb, loss_fn):
    o32, _ = _oracle(om, hb, loss_fn, torch.float32)
    o64, mags = _oracle(om, hb, loss_fn, torch.float64)
    return o32, o64, mags


# ---------------------------------------------------------------------------------------------------------------------
# 1. the hand-built batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_fn", ["cross_entropy", "l1"])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_hand_built_batch_matches_the_referee(L, loss_fn):
    hb = _collate(_hand_graphs(loss_fn))
    assert hb["virtual"].ptr.diff().tolist() == [1, 3, 2, 2, 4]
    om, pm = _models(9, 16, 10, L, "relu", seed=L)
    assert sum(q.numel() for q in pm.parameters()) == {1: 442 + 992, 2: 442 + 992 + 1664, 3: 4762}[L]
    hbd = hb.to(DEV)
    assert pm.supported(hbd)
    step = _run_step(pm, hbd, loss_fn)
    o32, o64, mags = _references(om, hb, loss_fn)
    _check_all(_step_outputs(step, pm), o32, o64, mags, L, f"hand L={L} {loss_fn}")
    if L == 3:      # the point of the feature: a virtual-side parameter of layer 0 trains
        g = _step_outputs(step, pm)["convs.0.convs.local__to__virtual.lin_src.weight"]
        assert float(g.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. Peptides-shaped batches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H,act", [(16, 16, "relu"), (16, 16, "elu"), (9, 32, "tanh"), (9, 32, "identity")])
def test_peptides_shaped_batch_matches_the_referee(F, H, act):
    hs = _peptides(4, 16, seed=H + len(act), F=F, max_nodes=250 if H == 32 else None)
    hb = _collate(hs)
    om, pm = _models(F, H, 10, 3, act, seed=H)
    hbd = hb.to(DEV)
    assert pm.resident_reason(hbd) is None
    step = _run_step(pm, hbd, "cross_entropy")
    o32, o64, mags = _references(om, hb, "cross_entropy")
    _check_all(_step_outputs(step, pm), o32, o64, mags, 3, f"peptides F={F} H={H} {act}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. layered and one-launch agreement
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_only_equals_the_step_below_the_lds_opt_in_line():
    """Graphs of at most 100 nodes: about 43 KB of LDS at H = 16, L = 3, within the 64 KB a launch gets without asking
    (every other forward-only launch of this file is above that line; the step has cases on both sides)."""
    hb = _collate(_peptides(4, 16, seed=3, max_nodes=100))
    _, pm = _models(9, 16, 10, 3, "elu", seed=7)
    hbd = hb.to(DEV)
    assert pm.resident_reason(hbd) is None
    step = _run_step(pm, hbd, "cross_entropy")
    pm.engine = "resident"
    with torch.no_grad():
        fwd = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
    torch.cuda.synchronize()
    assert pm.last_engine == "resident" and int(hbd._resident_meta.flag.item()) == 0
    assert torch.equal(fwd, step.pred)


def test_layered_step_passes_the_referee_and_forward_only_equals_the_step():
    from graph_hscn.loss import criterion
    hb = _collate(_peptides(4, 16, seed=3) + _hand_graphs("cross_entropy")[:2])
    om, pm = _models(9, 16, 10, 3, "elu", seed=7)
    hbd = hb.to(DEV)
    o32, o64, mags = _references(om, hb, "cross_entropy")
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    pm.zero_grad(set_to_none=True)
    pm.engine = "auto"
    pred = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
    assert pm.last_engine == "layered"
    loss, score = criterion("cross_entropy", pred, hbd["local"].y)
    loss.backward()
    lay = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "score": score.detach()}
    for q in pm.parameters():
        if q.grad is not None:
            lay[names[id(q)]] = q.grad
    _check_all(lay, o32, o64, mags, 3, "layered")
    pm.engine = "resident"
    with pytest.raises(RuntimeError, match=r"\('virtual', 'to', 'local'\)"):
        pm(hbd.x_dict, hbd.edge_index_dict, hbd)                      # gradients on: the autograd launches refuse
    pm.compute_virtual = False
    with pytest.raises(ValueError, match="compute_virtual"):
        pm(hbd.x_dict, hbd.edge_index_dict, hbd)
    pm.compute_virtual = True
    step = _run_step(pm, hbd, "cross_entropy")
    _check_all(_step_outputs(step, pm), o32, o64, mags, 3, "step")
    pm.keep_virtual = True
    with torch.no_grad():
        fwd = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
        assert pm.last_engine == "resident"
        xv = pm.last_virtual
        pm.engine = "layered"
        lay_pred = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
    torch.cuda.synchronize()
    assert int(hbd._resident_meta.flag.item()) == 0
    assert torch.equal(fwd, step.pred)
    assert _refereed(fwd, lay_pred, o64["pred"], "forward-only vs layered")
    keep = {}
    m64 = copy.deepcopy(om).double()
    x_dict, eid = _ref_inputs(hb, torch.float64)
    with torch.no_grad():
        m64(x_dict, eid, hb["local"].batch, hb.num_graphs, keep=keep)
        k32 = {}
        x32, _ = _ref_inputs(hb, torch.float32)
        copy.deepcopy(om)(x32, eid, hb["local"].batch, hb.num_graphs, keep=k32)
    assert _refereed(xv, k32["virtual"], keep["virtual"], "final virtual features")


# ---------------------------------------------------------------------------------------------------------------------
# 4. properties
# ---------------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical_and_a_graph_does_not_see_its_batch():
    hs = _peptides(3, 16, seed=11) + _hand_graphs("cross_entropy")
    _, pm = _models(9, 16, 10, 3, "relu", seed=11)
    step = _run_step(pm, _collate(hs).to(DEV), "cross_entropy")
    g0, p0 = step.grads.clone(), step.pred.clone()
    step.run()
    torch.cuda.synchronize()
    assert torch.equal(step.grads, g0) and torch.equal(step.pred, p0)
    for i in (0, 3, 6):
        alone = _run_step(pm, _collate([hs[i]]).to(DEV), "cross_entropy")
        assert torch.equal(alone.pred[0], p0[i]), i
    # the three-relation model has no gradient there; this one does
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    got = {names[id(q)]: g for q, g in step.param_grads}
    assert float(got["convs.0.convs.local__to__virtual.lin_src.weight"].abs().max()) > 0.0
    ref = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3).to(DEV)
    ref.engine = "layered"
    hbd = _collate(hs).to(DEV)
    TF.binary_cross_entropy_with_logits(ref(hbd.x_dict, hbd.edge_index_dict, hbd), hbd["local"].y).backward()
    assert ref.convs[0].convs["local__to__virtual"].lin_src.weight.grad is None


def test_accumulating_step_is_the_sum_of_plain_steps():
    from graph_hscn.step import VLResidentTrainStep
    hbd = _collate(_peptides(6, 16, seed=4)).to(DEV)
    _, pm = _models(9, 16, 10, 3, "tanh", seed=4)
    plain = VLResidentTrainStep(pm, hbd, "cross_entropy")
    acc = VLResidentTrainStep(pm, hbd, "cross_entropy", accumulate=True)
    torch.manual_seed(1)
    deltas = [[torch.randn_like(q) * 0.05 for q in pm.parameters()] for _ in range(3)]
    state = copy.deepcopy(pm.state_dict())
    gs, losses = [], []
    for d in deltas:
        with torch.no_grad():
            for q, dq in zip(pm.parameters(), d):
                q.add_(dq)
        plain.run()
        gs.append(plain.grads[:plain.P].clone())
        losses.append(plain.loss.clone())
    pm.load_state_dict(state)
    acc.grads.zero_()
    for d in deltas:
        with torch.no_grad():
            for q, dq in zip(pm.parameters(), d):
                q.add_(dq)
        acc.run()
    torch.cuda.synchronize()
    assert grads_close(acc.grads[:acc.P], (gs[0] + gs[1]) + gs[2])
    assert torch.equal(acc.loss, losses[-1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. loops
# ---------------------------------------------------------------------------------------------------------------------
def _loop_model():
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(0)
    return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, 16, 10, 3, vl_conv="GAT").to(DEV)


def test_fit_resident_equals_train_epoch_and_device_evaluator_equals_eval_epoch():
    """fit_resident on 40 graphs, B = 8, one epoch, AdamW, batch_accumulation 2, clipping, against train.train_epoch
    replaying the same order on the layered path: the tolerance of
    test_fit_resident_mpnn_equals_eager_step_loop_and_train_epoch (2e-4 relative to each parameter's magnitude)."""
    from graph_hscn.config.config import OPTIM_DICT, OptimConfig, TrainingConfig
    from graph_hscn.data import DataLoader
    from graph_hscn.metrics import eval_ap_hip
    from graph_hscn.train import train as T
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train_resident import fit_resident
    graphs = _peptides(52, 16, seed=31)
    train, val = graphs[:40], graphs[40:]
    B, k = 8, 2
    tc = TrainingConfig("hscn", "cross_entropy", "ap", epochs=1, eval_period=1, patience=50)
    cfg = OptimConfig("adamW", batch_accumulation=k, clip_grad_norm=True, lr=0.01)
    model = _loop_model()
    orders, evals = [], []
    hist = fit_resident(None, cfg, tc, train, None, model, batch_size=B, epoch_orders=orders,
                        eval_graphs=(val, val), metric="ap", eval_history=evals)
    assert len(hist) == 1 and len(orders) == 1
    lay = _loop_model()
    lay.engine = "layered"
    topt = OPTIM_DICT["adamW"](lay.parameters(), lr=0.01, weight_decay=cfg.weight_decay)
    loader = DataLoader([train[j] for j in orders[0].tolist()], batch_size=B)
    l_loss, _ = T.train_epoch(0, None, loader, lay, topt, "cross_entropy", None, k, True)
    print("epoch loss", hist[0][0], "layered", l_loss)
    assert abs(hist[0][0] - l_loss) <= 2e-4 * max(1.0, abs(l_loss))
    d = max(float((a - b_).detach().abs().max()) / max(1.0, float(b_.detach().abs().max()))
            for a, b_ in zip(model.parameters(), lay.parameters()))
    assert d <= 2e-4, d
    for q in model.vl_dead_params():
        assert q.grad is None
    # evaluation on the device against eval_epoch on a host loader (12 graphs: one full batch and a tail of 4)
    ev = DeviceEvaluator(val, model, "cross_entropy", B, "ap")
    loss_d, ap_d = ev.evaluate()
    assert model.last_engine == "resident"
    model.engine = "layered"
    loss_h, ap_h = T.eval_epoch(0, None, DataLoader(val, batch_size=B), model, "cross_entropy", eval_ap_hip, "Validation")
    print("eval", loss_d, ap_d, "host", loss_h, ap_h)
    assert abs(loss_d - loss_h) <= 1e-5 * max(1.0, abs(loss_h))
    assert abs(ap_d - ap_h) <= 1e-6
    assert evals and abs(evals[0][2] - loss_d) <= 1e-5 * max(1.0, abs(loss_d))


# ---------------------------------------------------------------------------------------------------------------------
# 6. envelope and fallback
# ---------------------------------------------------------------------------------------------------------------------
def _envelope_cases():
    from graph_hscn.data import Data
    hs = _peptides(2, 4, seed=1)
    g = torch.Generator().manual_seed(2)
    big = _hetero([Data(x=torch.randn(3000, 9, generator=g), edge_index=torch.randint(0, 3000, (2, 9000), generator=g),
                        y=torch.zeros(1, 10))], [np.random.default_rng(2).integers(0, 4, 3000)], 4)
    return {"F_gt_H": (17, 16, _peptides(2, 4, seed=1, F=17)), "H64": (9, 64, hs), "n3000": (9, 16, big)}


@pytest.mark.parametrize("case", ["F_gt_H", "H64", "n3000"])
def test_envelope_and_fallback(case):
    from graph_hscn.step import VLResidentTrainStep
    F, H, hs = _envelope_cases()[case]
    _, pm = _models(F, H, 10, 2, "relu", seed=1)
    pm.eval()
    hbd = _collate(hs).to(DEV)
    assert not pm.supported(hbd) and isinstance(pm.resident_reason(hbd), str)
    with pytest.raises(RuntimeError, match="does not take"):
        VLResidentTrainStep(pm, hbd, "cross_entropy")
    with torch.no_grad():
        pm.engine = "layered"
        ref = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
        pm.engine = "resident"
        with pytest.raises(RuntimeError, match="does not qualify"):
            pm(hbd.x_dict, hbd.edge_index_dict, hbd)
        pm.engine = "auto"
        out = pm(hbd.x_dict, hbd.edge_index_dict, hbd)
        assert pm.last_engine == "layered"
        assert torch.equal(out, ref)


def test_an_lv_target_outside_its_graph_is_flagged_not_followed():
    from graph_hscn.step import VLResidentTrainStep
    hb = _collate(_peptides(3, 4, seed=9))
    lo = int(hb[LV].ptr32[1])                       # graph 1's first lv edge: point it at graph 2's first cluster
    hb[LV].edge_index[1, lo] = int(hb["virtual"].ptr[2])
    _, pm = _models(9, 16, 10, 2, "relu", seed=9)
    step = VLResidentTrainStep(pm, hb.to(DEV), "cross_entropy")
    step.run()
    torch.cuda.synchronize()
    assert int(step.flag.item()) & 2
    assert bool(torch.isfinite(step.grads).all())
    with pytest.raises(IndexError):
        step.check()
