"""The MPNN baseline's one-launch training step and forward-only launch (include/hscn.h: hscn_mpnn_*) against the
CPU oracle (oracle.models.MPNN, reference model/mpnn.py:13-62 with GCNConv), refereed by the same oracle in float64:
the kernel and the float32 oracle are two different float32 roundings of one real-valued function, so the check is,
in max norm over each output,
    |HIP - f64|  <=  2 |oracle_f32 - f64| + 8 ulp(scale),      ulp(scale) = 2^-23 max|f64|
(tests/test_gpu_full_size.py states the same bar for the HSCN step)."""
import copy

import pytest
import torch
import torch.nn.functional as TF

from oracle import models as OM
from tests.helpers import DEV

pytestmark = pytest.mark.gpu


def _graphs(name, B, seed):
    from graph_hscn.loader.synthetic import make_dataset
    return make_dataset(name, B, seed=seed)


def _batch(graphs):
    from graph_hscn.data import Batch
    b = Batch.from_data_list(graphs)
    b.x = b.x.float()
    return b


def _dev(b):
    d = b.to(DEV)
    d.x = d.x.float().contiguous()
    return d


def _models(F, H, C, L, act, p, seed):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(seed)
    om = OM.MPNN(OM.ACT[act], F, H, C, L, p)
    with torch.no_grad():
        for n_, q in om.named_parameters():
            if n_.endswith("bias"):
                q.normal_(0, 0.1)
    pm = MPNN(CONV_DICT["gcn"], ACT_DICT[act], F, H, C, L, p).to(DEV)
    pm.load_state_dict(om.state_dict())
    return om, pm


def _masks(N, H, L, p, seed):
    """What nn.functional.dropout keeps in each hidden layer for layer seeds seed, seed + 1, ..."""
    from graph_hscn.nn import functional as Fh
    ones = torch.ones(N, H, device=DEV)
    return [(Fh.dropout(ones, p=p, training=True, seed=seed + i) != 0).float().cpu() for i in range(L - 1)]


def _oracle(om, b, loss_fn, masks, dtype):
    m = copy.deepcopy(om).to(dtype)
    m.zero_grad(set_to_none=True)
    pred = m(b.x.to(dtype), b.edge_index, b.batch, b.num_graphs,
             masks=None if masks is None else [mk.to(dtype) for mk in masks])
    y = b.y.to(dtype)
    loss = TF.binary_cross_entropy_with_logits(pred, y) if loss_fn == "cross_entropy" else TF.l1_loss(pred, y)
    loss.backward()
    out = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "score": torch.sigmoid(pred.detach())}
    for n_, q in m.named_parameters():
        out[n_] = q.grad
    return out


def _refereed(hip, o32, o64, what, k=2.0, ulps=8.0):
    hip, o32, o64 = (t.detach().cpu().double() for t in (hip, o32, o64))
    e_hip = float((hip - o64).abs().max())
    e_o32 = float((o32 - o64).abs().max())
    ulp = 2.0 ** -23 * float(o64.abs().max())
    ok = e_hip <= k * e_o32 + ulps * ulp
    if not ok:
        print(f"[f64 referee] {what}: |HIP-f64|={e_hip:.3e} |oracle32-f64|={e_o32:.3e} ulp(scale)={ulp:.3e}")
    return ok


def _step_outputs(step, pm):
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    out = {"pred": step.pred, "loss": step.loss.reshape(1), "score": step.score}
    for q, g in step.param_grads:
        out[names[id(q)]] = g
    return out


def _check_all(got, o32, o64, tag):
    bad = [k for k in o64 if not _refereed(got[k], o32[k], o64[k], f"{tag} {k}")]
    assert not bad, (tag, bad)


CASES = ([("peptides_func", B, "relu", 0.0) for B in (1, 32, 128)]
         + [("peptides_struct", B, "relu", 0.0) for B in (1, 32, 128)]
         + [("peptides_func", 32, act, p) for act in ("relu", "elu", "identity", "tanh") for p in (0.0, 0.2)]
         + [("peptides_struct", 128, "tanh", 0.2), ("peptides_struct", 32, "elu", 0.2)])


@pytest.mark.parametrize("name,B,act,p,H", [c + (16,) for c in CASES] + [("peptides_func", 32, "relu", 0.2, 32),
                                                                          ("peptides_struct", 32, "tanh", 0.2, 32)])
def test_step_matches_oracle_with_f64_referee(name, B, act, p, H):
    from graph_hscn.step import MPNNResidentTrainStep
    graphs = _graphs(name, B, seed=B + 7)
    if H == 32:           # (H = 32 holds graphs up to ~270 nodes in LDS: the Peptides graphs that small)
        graphs = [g for g in _graphs(name, 4 * B, seed=B + 7) if g.num_nodes <= 250][:B]
    b = _batch(graphs)
    C = b.y.size(1)
    loss_fn = "cross_entropy" if name == "peptides_func" else "l1"
    om, pm = _models(9, H, C, 3, act, p, seed=B)
    pm.train()
    pm.dropout_seed = 1234
    bd = _dev(b)
    assert pm.supported(bd)
    step = MPNNResidentTrainStep(pm, bd, loss_fn)
    step.run()
    torch.cuda.synchronize()
    step.check()
    masks = _masks(b.x.size(0), H, 3, p, 1234) if p > 0 else None
    o32 = _oracle(om, b, loss_fn, masks, torch.float32)
    o64 = _oracle(om, b, loss_fn, masks, torch.float64)
    _check_all(_step_outputs(step, pm), o32, o64, f"{name} B={B} {act} p={p} H={H}")


def test_dropout_contract_and_layered_agreement():
    """Step t draws nn.functional.dropout's masks at seed0 + (L-1) t + i; the layered MPNN with dropout_seed =
    seed0 + (L-1) t draws the same ones (so it agrees with the step within the referee bound)."""
    from graph_hscn.loss import criterion
    from graph_hscn.step import MPNNResidentTrainStep
    L, p, seed0 = 3, 0.2, 987654321
    b = _batch(_graphs("peptides_func", 16, seed=3))
    om, pm = _models(9, 16, 10, L, "relu", p, seed=3)
    pm.train()
    bd = _dev(b)
    step = MPNNResidentTrainStep(pm, bd, "cross_entropy", seed0=seed0)
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    preds = []
    for t in range(2):
        step.run()
        torch.cuda.synchronize()
        step.check()
        assert int(step.step_word.item()) == t + 1
        preds.append(step.pred.clone())
        masks = _masks(b.x.size(0), 16, L, p, seed0 + (L - 1) * t)
        o32 = _oracle(om, b, "cross_entropy", masks, torch.float32)
        o64 = _oracle(om, b, "cross_entropy", masks, torch.float64)
        _check_all(_step_outputs(step, pm), o32, o64, f"step t={t}")
        # the layered model with the step's seed
        pm.dropout_seed = seed0 + (L - 1) * t
        pm.engine = "layered"
        pm.zero_grad(set_to_none=True)
        pred = pm(bd)
        loss, _ = criterion("cross_entropy", pred, bd.y)
        loss.backward()
        lay = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "score": torch.sigmoid(pred.detach())}
        for q in pm.parameters():
            lay[names[id(q)]] = q.grad
        _check_all(_step_outputs(step, pm), lay, o64, f"step vs layered t={t}")
    assert not torch.equal(preds[0], preds[1])


def test_captured_replays_draw_new_masks():
    from graph_hscn.step import MPNNResidentTrainStep
    L, p, seed0 = 3, 0.2, 42
    b = _batch(_graphs("peptides_func", 8, seed=5))
    om, pm = _models(9, 16, 10, L, "tanh", p, seed=5)
    pm.train()
    step = MPNNResidentTrainStep(pm, _dev(b), "cross_entropy", seed0=seed0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step.run()                                   # warm-up: t = 0
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step.run()
    preds = []
    for t in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(step.step_word.item()) == t + 1
        preds.append(step.pred.clone())
        masks = _masks(b.x.size(0), 16, L, p, seed0 + (L - 1) * t)
        o32 = _oracle(om, b, "cross_entropy", masks, torch.float32)
        o64 = _oracle(om, b, "cross_entropy", masks, torch.float64)
        _check_all(_step_outputs(step, pm), o32, o64, f"replay t={t}")
    step.check()
    assert not torch.equal(preds[0], preds[1])


def _edge_case_graphs():
    from graph_hscn.data import Data
    g = torch.Generator().manual_seed(11)
    out = []
    # explicit and doubled self loops
    ei = torch.randint(0, 40, (2, 120), generator=g)
    ei = torch.cat([ei, torch.tensor([[3, 3, 5, 7, 7, 7], [3, 3, 5, 7, 7, 7]])], 1)
    out.append(Data(x=torch.randn(40, 9, generator=g), edge_index=ei, y=(torch.rand(1, 10, generator=g) < .5).float()))
    # isolated nodes (30 .. 49 have no edge)
    ei = torch.randint(0, 30, (2, 80), generator=g)
    out.append(Data(x=torch.randn(50, 9, generator=g), edge_index=ei, y=(torch.rand(1, 10, generator=g) < .5).float()))
    # one node with in-degree 20 and out-degree 20 (beyond six neighbours)
    ei = torch.randint(0, 60, (2, 150), generator=g)
    hub = torch.stack([torch.arange(1, 21), torch.zeros(20, dtype=torch.long)])
    ei = torch.cat([ei, hub, hub.flip(0)], 1)
    out.append(Data(x=torch.randn(60, 9, generator=g), edge_index=ei, y=(torch.rand(1, 10, generator=g) < .5).float()))
    # Peptides' largest graph: 444 nodes, in-degree ~6
    src = torch.randint(0, 444, (2664,), generator=g)
    dst = torch.arange(444).repeat_interleave(6)
    out.append(Data(x=torch.randint(0, 20, (444, 9), generator=g).float(), edge_index=torch.stack([src, dst]),
                    y=(torch.rand(1, 10, generator=g) < .5).float()))
    return out


@pytest.mark.parametrize("case", ["loops", "isolated", "hub", "n444", "all"])
def test_structure_edge_cases_match_layered(case):
    from graph_hscn.loss import criterion
    from graph_hscn.step import MPNNResidentTrainStep
    gs = _edge_case_graphs()
    pick = {"loops": [0], "isolated": [1], "hub": [2], "n444": [3], "all": [0, 1, 2, 3]}[case]
    b = _batch([gs[i] for i in pick])
    om, pm = _models(9, 16, 10, 3, "relu", 0.0, seed=len(pick))
    bd = _dev(b)
    step = MPNNResidentTrainStep(pm, bd, "cross_entropy")
    step.run()
    torch.cuda.synchronize()
    step.check()
    names = {id(q): n_ for n_, q in pm.named_parameters()}
    pm.zero_grad(set_to_none=True)
    pred = pm(bd)
    loss, _ = criterion("cross_entropy", pred, bd.y)
    loss.backward()
    lay = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "score": torch.sigmoid(pred.detach())}
    for q in pm.parameters():
        lay[names[id(q)]] = q.grad
    o64 = _oracle(om, b, "cross_entropy", None, torch.float64)
    _check_all(_step_outputs(step, pm), lay, o64, f"edge case {case} vs layered")
    o32 = _oracle(om, b, "cross_entropy", None, torch.float32)
    _check_all(_step_outputs(step, pm), o32, o64, f"edge case {case} vs oracle")


def _wide(b, F):
    """The same batch with F feature columns (the first nine repeated)."""
    import copy as _copy
    w = _copy.copy(b)
    w.x = b.x.repeat(1, (F + 8) // 9)[:, :F].contiguous()
    return w


def _unsupported_cases():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.data import Batch, Data
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.nn.conv import GATConv, GraphConv
    b = _batch(_graphs("peptides_func", 4, seed=1))
    g = torch.Generator().manual_seed(2)
    big = Batch.from_data_list([Data(x=torch.randn(3000, 9, generator=g),
                                     edge_index=torch.randint(0, 3000, (2, 9000), generator=g),
                                     y=torch.zeros(1, 10))])
    mc = Batch.from_data_list([Data(x=g0.x.float(), edge_index=g0.edge_index, y=torch.tensor([i % 10]))
                               for i, g0 in enumerate(_graphs("peptides_func", 4, seed=1))])
    gcn, relu = CONV_DICT["gcn"], ACT_DICT["relu"]
    torch.manual_seed(0)
    return {
        "layer_norm": (MPNN(gcn, relu, 9, 16, 10, 3, 0.0, use_layer_norm=True), b),
        "gat": (MPNN(lambda i, o: GATConv(i, o, add_self_loops=False), relu, 9, 16, 10, 3), b),
        "graphconv": (MPNN(lambda i, o: GraphConv(i, o), relu, 9, 16, 10, 3), b),
        "batch_norm": (MPNN(gcn, relu, 9, 16, 10, 3, 0.0, use_batch_norm=True, use_layer_norm=True), b),
        "F_gt_H": (MPNN(gcn, relu, 17, 16, 10, 3), _wide(b, 17)),
        "over_lds": (MPNN(gcn, relu, 9, 16, 10, 3), big),
        "multiclass": (MPNN(gcn, relu, 9, 16, 10, 3), mc),
    }


@pytest.mark.parametrize("case", ["layer_norm", "batch_norm", "gat", "graphconv", "F_gt_H", "over_lds", "multiclass"])
def test_envelope_and_fallback(case):
    pm, b = _unsupported_cases()[case]
    pm = pm.to(DEV).eval()
    bd = _dev(b)
    with torch.no_grad():
        pm.engine = "layered"
        ref = pm(bd)
        assert pm.last_engine == "layered"
        assert not pm.supported(bd)
        assert isinstance(pm.resident_reason(bd), str)
        pm.engine = "resident"
        with pytest.raises(RuntimeError, match="does not qualify"):
            pm(bd)
        pm.engine = "auto"
        out = pm(bd)
        assert pm.last_engine == "layered"
        assert torch.equal(out, ref)


def test_forward_only_equals_train_step_pred_and_eval_epoch():
    from graph_hscn.data import DataLoader
    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train.train import eval_epoch
    graphs = _graphs("peptides_func", 70, seed=9)
    b = _batch(graphs[:32])
    om, pm = _models(9, 16, 10, 3, "tanh", 0.0, seed=9)
    bd = _dev(b)
    step = MPNNResidentTrainStep(pm, bd, "cross_entropy")
    step.run()
    pm.eval()
    pm.engine = "resident"
    with torch.no_grad():
        pred = pm(bd)
    torch.cuda.synchronize()
    assert pm.last_engine == "resident"
    assert int(pm._resident_flag.item()) == 0
    assert torch.equal(pred, step.pred)
    # eval_epoch (torch.no_grad) through the forward-only launch against the layered engine, refereed per batch mean
    loader = DataLoader(graphs, batch_size=32, shuffle=False)
    r_loss, _ = eval_epoch(0, None, loader, pm, "cross_entropy", None, "Validation")
    assert pm.last_engine == "resident"
    pm.engine = "layered"
    l_loss, _ = eval_epoch(0, None, loader, pm, "cross_entropy", None, "Validation")
    assert pm.last_engine == "layered"
    o64 = []
    for i in range(0, 70, 32):
        bb = _batch(graphs[i:i + 32])
        om64 = copy.deepcopy(om).double().eval()
        with torch.no_grad():
            pr = om64(bb.x.double(), bb.edge_index, bb.batch, bb.num_graphs)
            o64.append(TF.binary_cross_entropy_with_logits(pr, bb.y.double()))
    ref = float(torch.stack(o64).mean())
    assert _refereed(torch.tensor([r_loss]), torch.tensor([l_loss]), torch.tensor([ref]), "eval_epoch loss")


def test_forward_only_equals_train_step_pred_below_the_lds_opt_in_line():
    """Graphs of at most 150 nodes: at most 52 KB of LDS at H = 16, L = 3, within the 64 KB a launch gets without asking
    (every other forward-only launch of this file is above that line; the step has cases on both sides)."""
    from graph_hscn.step import MPNNResidentTrainStep
    graphs = [g for g in _graphs("peptides_func", 70, seed=9) if g.num_nodes <= 150][:16]
    assert len(graphs) == 16
    _, pm = _models(9, 16, 10, 3, "tanh", 0.0, seed=9)
    bd = _dev(_batch(graphs))
    step = MPNNResidentTrainStep(pm, bd, "cross_entropy")
    step.run()
    pm.eval()
    pm.engine = "resident"
    with torch.no_grad():
        pred = pm(bd)
    torch.cuda.synchronize()
    assert pm.last_engine == "resident" and int(pm._resident_flag.item()) == 0
    assert torch.equal(pred, step.pred)


def test_accumulating_step_is_the_sum_of_plain_steps():
    from graph_hscn.step import MPNNResidentTrainStep
    b = _batch(_graphs("peptides_struct", 24, seed=4))
    _, pm = _models(9, 16, 11, 3, "elu", 0.0, seed=4)
    bd = _dev(b)
    plain = MPNNResidentTrainStep(pm, bd, "l1")
    acc = MPNNResidentTrainStep(pm, bd, "l1", accumulate=True)
    gs, losses = [], []
    torch.manual_seed(1)
    deltas = [[torch.randn_like(q) * 0.05 for q in pm.parameters()] for _ in range(3)]
    state = copy.deepcopy(pm.state_dict())
    for d in deltas:                      # k = 3 micro-steps at three points of the weights
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
    want = (gs[0] + gs[1]) + gs[2]
    assert torch.equal(acc.grads[:acc.P], want)
    assert torch.equal(acc.loss, losses[-1])


def test_forward_only_loss_equals_train_step_loss():
    """hscn_mpnn_forward with a target: the per-graph loss rows and their one-column fold give the train step's loss
    (p = 0) bit for bit -- the same loss row, the same summation tree."""
    from graph_hscn import _hip
    from graph_hscn.engine import _ptr_table
    from graph_hscn.step import MPNNResidentTrainStep
    for name, C, fn, kind in (("peptides_func", 10, "cross_entropy", 0), ("peptides_struct", 11, "l1", 1)):
        b = _batch(_graphs(name, 40, seed=C))
        _, pm = _models(9, 16, C, 3, "relu", 0.0, seed=C)
        bd = _dev(b)
        step = MPNNResidentTrainStep(pm, bd, fn)
        step.run()
        params = [q.detach().contiguous() for q in pm.resident_params()]
        pred = torch.empty(40, C, device=DEV)
        score = torch.empty(40, C, device=DEV)
        rows = torch.empty(40, device=DEV)
        loss = torch.empty(1, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        _hip.call("hscn_mpnn_forward", _hip.ptr(bd.x), _hip.ptr(bd.edge_index), bd.edge_index.size(1),
                  _hip.ptr(bd.ptr32), _hip.ptr(bd.eptr32), bd.x.size(0), 40, 9, 16, 3, C, _hip.ACT["relu"],
                  _ptr_table(params), bd.max_nodes, bd.max_edges, _hip.ptr(bd.y), kind, 1.0 / (40 * C),
                  _hip.ptr(pred), _hip.ptr(score), _hip.ptr(rows), _hip.ptr(loss), _hip.ptr(flag), _hip.stream())
        torch.cuda.synchronize()
        assert int(flag.item()) == 0
        assert torch.equal(pred, step.pred) and torch.equal(score, step.score)
        assert torch.equal(loss.view(()), step.loss), (name, float(loss), float(step.loss))
        assert torch.equal(rows, step.partials[:, step.P])


def test_device_graph_dataset_gather_is_batch_from_data_list():
    from graph_hscn.loader.device_dataset import DeviceGraphDataset
    graphs = _graphs("peptides_struct", 30, seed=21)
    ds = DeviceGraphDataset(graphs, DEV, 8)
    for ids in ([3, 17, 0, 29, 5, 11, 12, 2], [29, 28, 27, 1, 0, 4, 8, 9]):
        out = ds.gather(torch.tensor(ids, device=DEV))
        torch.cuda.synchronize()
        ref = _batch([graphs[i] for i in ids])
        n, e = int(ref.ptr[-1]), ref.edge_index.size(1)
        assert torch.equal(out.x[:n].cpu(), ref.x)
        assert torch.equal(out.edge_index[:, :e].cpu(), ref.edge_index)
        assert torch.equal(out.batch[:n].cpu(), ref.batch)
        assert torch.equal(out.ptr.cpu(), ref.ptr) and torch.equal(out.ptr32.cpu(), ref.ptr32)
        assert torch.equal(out.eptr32.cpu(), ref.eptr32) and torch.equal(out.y.cpu(), ref.y)
    ds.check()


def test_device_graph_dataset_self_walking_epoch_equals_explicit_gathers():
    """gather_next() serves perm[0:B], perm[B:2B] of the epoch new_epoch() drew: bit for bit what gather() builds
    from those slices (the homogeneous counterpart of test_gpu_device_dataset's test of the same name)."""
    from graph_hscn.loader.device_dataset import DeviceGraphDataset
    B = 8
    ds = DeviceGraphDataset(_graphs("peptides_func", 20, seed=23), DEV, B)
    with pytest.raises(RuntimeError):
        ds.gather_next()
    def valid(out):       # (behind the batch's own nodes / edges the static buffers hold stale data)
        n, e = int(out.ptr32[-1]), int(out.eptr32[-1])
        return {"x": out.x[:n].clone(), "edge_index": out.edge_index[:, :e].clone(), "ptr32": out.ptr32.clone(),
                "eptr32": out.eptr32.clone(), "y": out.y.clone()}

    perm = ds.new_epoch(torch.Generator(device=DEV).manual_seed(4)).clone()
    got = [valid(ds.gather_next()) for _ in range(2)]
    for i in range(2):
        want = valid(ds.gather(perm[i * B:(i + 1) * B]))
        for f in want:
            assert torch.equal(got[i][f], want[f]), (i, f)
    assert not torch.equal(got[0]["y"], got[1]["y"])            # (two batches, not one batch twice)
    ds.check()


def _mpnn_model(p):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(0)
    m = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, 10, 3, p).to(DEV)
    m.dropout_seed = 777
    return m


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fit_resident_mpnn_equals_eager_step_loop_and_train_epoch(p, monkeypatch):
    """fit_resident(MPNN): 3 epochs, G % B != 0, AdamW, batch_accumulation 2, clipping.  Per-epoch losses and final
    parameters are bitwise those of an eager loop of MPNNResidentTrainStep.run() + FlatAdam over the same epoch orders
    (same gather, same tail handling); with p = 0 the run stays within 2e-4 (relative to each parameter's magnitude)
    of train.train_epoch on the layered model."""
    from graph_hscn.config.config import OPTIM_DICT, OptimConfig, TrainingConfig
    from graph_hscn.data import Batch, DataLoader
    from graph_hscn.loader.device_dataset import DeviceGraphDataset
    from graph_hscn.loss import criterion
    from graph_hscn.optim import FlatAdam
    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import train as T
    from graph_hscn.train.train_resident import CLIP_MAX_NORM, fit_resident, optimizer_steps_at
    graphs = _graphs("peptides_func", 50, seed=31)
    for g in graphs:
        g.x = g.x.float() * 3.0                    # gradient norms above 1: the clip engages
    G, B, k, epochs = 42, 8, 2, 3                  # 5 captured batches + a 2-graph eager tail
    train, loaders = graphs[:G], [DataLoader(graphs[G:46], batch_size=4), DataLoader(graphs[46:], batch_size=4)]
    tc = TrainingConfig("mpnn", "cross_entropy", "ap", epochs=epochs, eval_period=epochs, patience=50)
    cfg = OptimConfig("adamW", batch_accumulation=k, clip_grad_norm=True, lr=0.01)
    model = _mpnn_model(p)
    orders = []
    hist = fit_resident(None, cfg, tc, train, loaders, model, batch_size=B, epoch_orders=orders)
    assert len(hist) == epochs and len(orders) == epochs
    assert model.last_engine == "resident"        # (evaluation took the forward-only launch)

    # the eager loop: the same device gather, the step run eagerly, FlatAdam stepped where fit_resident steps it
    ref = _mpnn_model(p)
    ds = DeviceGraphDataset(train, DEV, B)
    step = MPNNResidentTrainStep(ref, ds.static.batch, "cross_entropy", accumulate=True)
    step.bind_grads()
    opt = FlatAdam.from_config("adamW", step.param_grads, step.grads, lr=0.01, weight_decay=cfg.weight_decay,
                               max_norm=CLIP_MAX_NORM, zero_grads=True)
    # CapturedStep's three warm-up runs and fit_resident's own counter: the step word the captured run started at
    step.step_word.fill_(3)
    steps, nb = G // B, G // B + 1
    losses = []
    for o in orders:
        od = o.to(DEV)
        ep = []
        for i in range(steps):
            ds.gather(od[i * B:(i + 1) * B].contiguous())
            step.run()
            if optimizer_steps_at(i, nb, k):
                opt.step()
            ep.append(step.loss.clone())
        hb = Batch.from_data_list([train[j] for j in o[steps * B:].tolist()]).to(DEV)
        hb.x = hb.x.float()
        ref.engine = "resident"
        opt.zero_grad(set_to_none=True)
        loss, _ = criterion("cross_entropy", ref(hb), hb.y)
        loss.backward()
        opt.step_from_autograd(accumulate=True)
        ep.append(loss.detach())
        losses.append(float(torch.stack(ep).mean()))
    assert [h[0] for h in hist] == losses
    for a, b_ in zip(model.parameters(), ref.parameters()):
        assert torch.equal(a, b_)

    if p == 0.0:    # against the reference-shaped loop on the layered model (torch's AdamW and clip_grad_norm_)
        lay = _mpnn_model(p)
        topt = OPTIM_DICT["adamW"](lay.parameters(), lr=0.01, weight_decay=cfg.weight_decay)
        for e, o in enumerate(orders):
            loader = DataLoader([train[j] for j in o.tolist()], batch_size=B)
            T.train_epoch(e, None, loader, lay, topt, "cross_entropy", None, k, True)
        d = max(float((a - b_).detach().abs().max()) / max(1.0, float(b_.detach().abs().max()))
                for a, b_ in zip(model.parameters(), lay.parameters()))
        assert d <= 2e-4, d
