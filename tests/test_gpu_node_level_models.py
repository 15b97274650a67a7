"""Node-level HSCN / MPNN on the device against the CPU oracle in float64, and ``train.train`` on per-node labels.

The oracle: ``oracle.models.HSCN.forward(..., keep=d)`` gives the final local features, the head is
``lin_2(activation(lin_1(d["local"])))`` on them; the MPNN's node-level output is its last convolution's.  With the
virtual -> local relation the oracle gets the fourth convolution tests/test_gpu_hscn_vl.py gives it.

Bound.  A whole model is a chain of kernels whose a-priori n and mag nobody has derived; what is compared is the
reference's own float32 error, as tests/test_gpu_hscn_vl.py does: |HIP - f64| <= 2 |oracle_f32 - f64| + 8 ulp(scale)
element-wise maxima, ulp(scale) = 2^-23 max |f64|.  Its teeth, each rejected by the same limit: the float64
prediction with the largest product of one ``lin_2`` row removed; the loss without the row of the largest w |logp|;
the gradients of the head (``lin_1``, ``lin_2``: weight and bias) and of every local -> local convolution (its
transform's weight, its bias) without the node of the largest contribution (weight: the outer product of the node's
output gradient and input; bias: the node's output gradient)."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import models as OM
from oracle import pyg_ops as P
from tests.helpers import DEV, drop_largest_product

pytestmark = pytest.mark.gpu

VL = ("virtual", "to", "local")
LV = ("local", "to", "virtual")


def _within(got, f64, o32, what, against=None):
    """``against``: the tensor to measure ``got`` against under the SAME limit (the dropped-term reference)."""
    got, f64, o32 = got.detach().cpu().double(), f64.detach().double(), o32.detach().double()
    ulp = 2.0 ** -23 * max(float(f64.abs().max()), 1e-30)
    lim = 2.0 * float((o32 - f64).abs().max()) + 8.0 * ulp
    d = float((got - (f64 if against is None else against.double())).abs().max())
    print(f"[node-level] {what}: |HIP-f64|={d:.3e} limit={lim:.3e}")
    return d <= lim


@functools.lru_cache(maxsize=None)
def _batches():
    """4 Peptides-shaped graphs with random node labels (C = 10); 2 pascalvoc_sp_node graphs (more rows than one
    workgroup of the head takes)."""
    from graph_hscn.data import HeteroBatch
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    out = {}
    for name, src, B, C, K in (("peptides", "peptides_func", 4, 10, 8), ("pascal", "pascalvoc_sp_node", 2, 21, 8)):
        graphs = make_dataset(src, B, seed=11)
        rng = np.random.default_rng(11)
        gen = torch.Generator().manual_seed(11)
        for g in graphs:
            g.x = torch.randn(g.num_nodes, g.x.size(1), generator=gen)
            if name == "peptides":
                g.y = torch.randint(0, C, (g.num_nodes,), generator=gen)
        hs = [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K) for g in graphs]
        out[name] = (HeteroBatch.from_data_list(hs), graphs, C)
    assert out["pascal"][0]["local"].x.size(0) > 256
    return out



def _models(F, H, C, L, vl, seed=0):
    from graph_hscn.config.config import ACT_DICT
    from graph_hscn.model.hscn import HSCN
    torch.manual_seed(seed)
    om = OM.HSCN("GAT", "GCN", "GCN", OM.ACT["relu"], F, H, C, L)
    if vl:
        for l, conv in enumerate(om.convs):
            fin = F if l == 0 else H
            conv.convs["virtual__to__local"] = P.GATConv((fin, fin), H)
    with torch.no_grad():
        for n_, q in om.named_parameters():
            if n_.endswith("bias"):
                q.normal_(0, 0.1)
    pm = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], F, H, C, L, vl_conv="GAT" if vl else None,
              task_level="node").to(DEV)
    assert sorted(pm.state_dict()) == sorted(om.state_dict())
    pm.load_state_dict(om.state_dict())
    return om, pm


def _oracle(om, hb, dtype, vl):
    """Node-level pred, the weighted loss and every parameter gradient (None where autograd leaves none)."""
    from graph_hscn.loss import batch_class_weights
    m = copy.deepcopy(om).to(dtype)
    m.zero_grad(set_to_none=True)
    kept = {}                                         # parameter name -> (input or None, output) of the module call

    def hook(weight, bias):
        def fn(mod, inp, out):
            out.retain_grad()
            if weight is not None:
                kept[weight] = (inp[0].detach(), out)
            if bias is not None:
                kept[bias] = (None, out)
        return fn

    hooks = [m.lin_1.register_forward_hook(hook("lin_1.weight", "lin_1.bias")),
             m.lin_2.register_forward_hook(hook("lin_2.weight", "lin_2.bias"))]
    for l, conv in enumerate(m.convs):
        ll = conv.convs["local__to__local"]
        name = f"convs.{l}.convs.local__to__local"
        hooks.append(ll.lin.register_forward_hook(hook(f"{name}.lin.weight", None)))
        hooks.append(ll.register_forward_hook(hook(None, f"{name}.bias")))
    eid = dict(hb.edge_index_dict)
    if vl:
        eid[VL] = eid[LV].flip(0)
    d = {}
    m({k: v.to(dtype) for k, v in hb.x_dict.items()}, eid, hb["local"].batch, hb.num_graphs, keep=d)
    hidden = m.activation(m.lin_1(d["local"]))
    pred = m.lin_2(hidden)
    y = hb["local"].y
    w = batch_class_weights(y, pred.size(1)).to(dtype)
    loss = TF.cross_entropy(pred, y, weight=w)
    loss.backward()
    for h in hooks:
        h.remove()
    out = {"pred": pred.detach(), "loss": loss.detach().reshape(1), "hidden": hidden.detach(),
           "W2": m.lin_2.weight.detach()}
    params = dict(m.named_parameters())
    for n_, q in params.items():
        out[n_] = q.grad
    # the dropped-term references
    logp = TF.log_softmax(pred.detach(), -1)
    terms = w[y] * -logp.gather(1, y[:, None]).squeeze(1)
    dropped = {"loss": ((terms.sum() - terms[terms.abs().argmax()]) / w[y].sum()).reshape(1)}
    for n_, (x_in, o) in kept.items():
        assert n_ in params and params[n_].grad is not None, n_
        g = o.grad
        if x_in is None:
            dropped[n_] = params[n_].grad - g[g.abs().max(1).values.argmax()]
        else:
            r = int((g.abs().max(1).values * x_in.abs().max(1).values).argmax())
            dropped[n_] = params[n_].grad - torch.outer(g[r], x_in[r])
    out["dropped"] = dropped
    return out


@pytest.mark.parametrize("route", ["fused", "layered"])
@pytest.mark.parametrize("vl", [False, True])
@pytest.mark.parametrize("name", ["peptides", "pascal"])
def test_hscn_node_level_against_the_oracle(name, vl, route):
    from graph_hscn.loss import criterion
    hb, _, C = _batches()[name]
    F = hb["local"].x.size(1)
    om, pm = _models(F, 16, C, 3, vl)
    o32, o64 = _oracle(om, hb, torch.float32, vl), _oracle(om, hb, torch.float64, vl)
    b = hb.to(DEV)
    pm.node_head.route = route
    pred = pm(b.x_dict, b.edge_index_dict, b)
    assert pred.shape == (hb["local"].x.size(0), C) and pm.last_engine == "layered"
    assert pm.node_head.last_route == route
    assert _within(pred, o64["pred"], o32["pred"], f"{name} vl={vl} pred")
    dropped = drop_largest_product(o64["pred"], o64["hidden"], o64["W2"].T,
                                   post=lambda r, o, t: float(o64["pred"][r, o]) - t)
    assert not _within(pred, o64["pred"], o32["pred"], "dropped lin_2 product", against=dropped)
    loss, score = criterion("weighted_cross_entropy", pred, b["local"].y)
    assert score.shape == pred.shape
    assert _within(loss.detach().reshape(1), o64["loss"], o32["loss"], f"{name} vl={vl} loss")
    assert not _within(loss.detach().reshape(1), o64["loss"], o32["loss"], "dropped loss row",
                       against=o64["dropped"]["loss"])
    loss.backward()
    live = toothed = 0
    for n_, q in pm.named_parameters():
        if o64[n_] is None:
            assert q.grad is None, f"{n_} cannot be reached by the prediction"
        else:
            assert q.grad is not None, n_
            assert _within(q.grad, o64[n_], o32[n_], f"{name} vl={vl} d/d{n_}")
            if n_ in o64["dropped"]:
                assert not _within(q.grad, o64[n_], o32[n_], f"dropped node of d/d{n_}", against=o64["dropped"][n_])
                toothed += 1
            live += 1
    assert live >= 4 + 2 * 3                                          # the head and the ll convolutions at least
    assert toothed == 4 + 2 * 3                                       # ... each with its dropped-term reference


def test_both_head_routes_give_the_model_the_same_prediction_within_the_bound():
    hb, _, C = _batches()["pascal"]
    om, pm = _models(hb["local"].x.size(1), 16, C, 3, False)
    o32, o64 = _oracle(om, hb, torch.float32, False), _oracle(om, hb, torch.float64, False)
    b = hb.to(DEV)
    for route in ("fused", "layered"):
        pm.node_head.route = route
        with torch.no_grad():
            pred = pm(b.x_dict, b.edge_index_dict, b)
        assert pm.node_head.last_route == route
        assert _within(pred, o64["pred"], o32["pred"], f"route {route}")


def test_mpnn_node_level_is_the_last_convolution_before_the_pool():
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.data import Batch
    from graph_hscn.model.mpnn import MPNN
    _, graphs, C = _batches()["peptides"]
    batch = Batch.from_data_list(graphs)
    torch.manual_seed(1)
    om = OM.MPNN(OM.ACT["relu"], 9, 16, C, 3)
    pm = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, 16, C, 3, task_level="node").to(DEV)
    pm.load_state_dict(om.state_dict())
    pm.eval()
    ref = {}
    for dtype in (torch.float32, torch.float64):
        m = copy.deepcopy(om).to(dtype).eval()
        x = batch.x.to(dtype)
        for i in range(m.num_layers - 1):
            x = m.activation(TF.relu(m.conv_layers[i](x, batch.edge_index)))
        ref[dtype] = m.conv_layers[-1](x, batch.edge_index).detach()
    b = batch.to(DEV)
    b.x = b.x.float()
    pred = pm(b)
    assert pred.shape == (batch.x.size(0), C)
    assert _within(pred, ref[torch.float64], ref[torch.float32], "mpnn node-level pred")
    pooled = P.global_mean_pool(ref[torch.float64], batch.batch, batch.num_graphs)
    assert pooled.shape != pred.shape                                   # (nothing was pooled)


@pytest.mark.parametrize("kind", ["hscn", "mpnn"])
def test_train_runs_a_node_level_model_and_scores_nodes(kind):
    from graph_hscn import metrics
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.data import DataLoader
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.model.mpnn import MPNN
    from graph_hscn.train.train import train
    graphs = make_dataset("pascalvoc_sp_node", 8, seed=2)
    C = 21
    torch.manual_seed(0)
    if kind == "hscn":
        rng = np.random.default_rng(2)
        data = [hetero_from_clusters(g, rng.integers(0, 8, g.num_nodes), 8) for g in graphs]
        model = HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 14, 16, C, 2, task_level="node").to(DEV)
    else:
        data = graphs
        model = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 14, 16, C, 3, task_level="node").to(DEV)
    loaders = [DataLoader(data[:4], 2, shuffle=False), DataLoader(data[4:6], 2, shuffle=False),
               DataLoader(data[6:], 2, shuffle=False)]
    nodes = sum(g.num_nodes for g in graphs[:4])
    for name, cpu_fn in (("f1_macro", metrics.eval_f1_macro), ("accuracy", metrics.eval_accuracy)):
        seen = []

        def metric_fn(y_true, y_pred):
            value = metrics.eval_hip(name)(y_true, y_pred)
            seen.append((y_true.cpu(), y_pred.cpu(), value))
            return value

        cfg = SimpleNamespace(epochs=2, eval_period=1, loss_fn="weighted_cross_entropy", patience=10, min_delta=0.0)
        opt = SimpleNamespace(optim_type="adam", lr=1e-2, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                              scheduler=None)
        history = train(None, opt, cfg, loaders, model, metric_fn)
        assert len(history) == 2 and all(np.isfinite(l) and np.isfinite(p) for l, p in history)
        assert len(seen) == 6                                           # train, validation, test per epoch
        assert seen[0][0].shape == (nodes,) and seen[0][1].shape == (nodes, C)      # metric rows are nodes
        for y_true, y_pred, value in seen:
            assert value == cpu_fn(y_true, y_pred)                      # the confusion matrix is integers: equal
        assert [p for _, p in history] == [seen[0][2], seen[3][2]]
