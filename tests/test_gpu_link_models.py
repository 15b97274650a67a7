"""Link-level HSCN / MPNN on the device: ``embed`` is the node-level model's forward, ``forward`` the pair decoder on it,
the BCE loss reaches the parameters the node-level loss reaches, and ``train.train`` reports a per-graph MRR.

The convolution stack and the node head under ``embed`` are tested where they were added; what a link-level model adds
is ``loss = BCE(pair_dot(z), edge_label)`` on the embedding z, and its gradient dL/dz is compared with the same
expression in float64 on the CPU on the same float32 z.  Bound, in the form of ``tests/helpers.check_f64``:
  s_p = <z_u, z_v>: |ds_p| <= D u A_p with A_p = sum_k |z_u,k| |z_v,k|                         (u = 2^-24)
  g_p = (sigmoid(s_p) - y_p) / P: sigmoid is 1/4-Lipschitz and evaluated to a few ulp of a value <= 1:
        |dg_p| <= (D u A_p / 4 + 4 u) / P =: u G_p
  dL/dz_i = sum over the incidences of i of g_p z_other:
        |error| <= (deg_i + 1) u sum |g_p| |z_other|  +  u sum G_p |z_other|
so n = 1 and mag = (deg_i + 1) sum |g_p| |z_other| + sum G_p |z_other| under F64_C.  Dropped term: the incidence with
the largest |g_p| |z_other|.

The training-loop test recomputes the embeddings with the final weights and ranks them on the CPU
(``metrics.link_rank_counts``) by scores that ``pair_dot`` itself gives for every ordered pair of a graph's nodes: the
float32 values the model ranks by, bit for bit, so no comparison can fall differently.  Another evaluation of the same
rows is not the same metric: two leaves of one parent whose hidden features the ReLU has zeroed get embeddings that
agree except in their last bits, their scores against any u differ by 2e-10 relative (3.3e-8 at 171.55 in the MPNN of
this test), float32 returns one value for both -- a tie, rank2 31 -- and float64 separates them -- rank2 32 -- which
moved the MRR by 3.8e-6; a float32 product in another summation order could fall either way."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import check_f64

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, D, K = 16, 16, 4
EPS64 = 2.0 ** -52


def _data(kind, num, seed):
    from graph_hscn.loader.hetero_data import hetero_from_clusters
    from graph_hscn.loader.synthetic import make_dataset
    graphs = make_dataset("pcqm_contact_link", num, seed=seed)
    if kind == "mpnn":
        return graphs
    rng = np.random.default_rng(seed)
    return [hetero_from_clusters(g, rng.integers(0, K, g.num_nodes), K, "link") for g in graphs]


def _model(kind, task_level, vl=None):
    from graph_hscn.config.config import ACT_DICT, CONV_DICT
    from graph_hscn.model.hscn import HSCN
    from graph_hscn.model.mpnn import MPNN
    torch.manual_seed(0)
    if kind == "hscn":
        return HSCN("GAT", "GCN", "GCN", ACT_DICT["relu"], 9, H, D, 2, vl_conv=vl, task_level=task_level).to(DEV)
    return MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, H, D, 3, task_level=task_level).to(DEV)


def _batch(kind, model, num=4, seed=3):
    from graph_hscn.train import batching
    return batching.collate(model, _data(kind, num, seed), DEV)


def _embed(kind, model, batch):
    return model.embed(batch.x_dict, batch.edge_index_dict, batch) if kind == "hscn" else model.embed(batch)


def _store(kind, batch):
    return batch["local"] if kind == "hscn" else batch


@pytest.mark.parametrize("kind,vl", [("hscn", None), ("hscn", "GAT"), ("mpnn", None)])
def test_embed_is_the_node_level_forward_and_forward_is_pair_dot_of_it(kind, vl):
    from graph_hscn.nn.head import pair_dot
    from graph_hscn.train import batching
    link, node = _model(kind, "link", vl), _model(kind, "node", vl)
    node.load_state_dict(link.state_dict())
    batch = _batch(kind, link)
    with torch.no_grad():
        z = _embed(kind, link, batch)
        want = node(batch.x_dict, batch.edge_index_dict, batch) if kind == "hscn" else node(batch)
        assert z.shape == (_store(kind, batch).num_nodes, D) and torch.equal(z, want)
        scores, labels = batching.forward(link, batch)
        again = batching.link_forward(link, batch)
        assert torch.equal(again[0], scores) and torch.equal(again[2], z) and not again[2].requires_grad
    pairs = _store(kind, batch).edge_label_index
    assert scores.shape == (pairs.size(1),) and torch.equal(labels, _store(kind, batch).edge_label)
    assert torch.equal(scores, pair_dot(z, pairs))
    assert torch.equal(batching.targets(link, batch), labels)
    assert link.last_engine == "layered"


@pytest.mark.parametrize("kind,vl", [("hscn", None), ("hscn", "GAT"), ("mpnn", None)])
def test_bce_gradients_reach_what_the_node_level_loss_reaches_and_match_float64_at_the_pair_head(kind, vl):
    from graph_hscn.loss import criterion
    from graph_hscn.nn.head import PairStructure, pair_dot
    from graph_hscn.train import batching
    link, node = _model(kind, "link", vl), _model(kind, "node", vl)
    node.load_state_dict(link.state_dict())
    batch = _batch(kind, link)
    scores, labels = batching.forward(link, batch)
    loss, _ = criterion("cross_entropy", scores, labels)
    loss.backward()
    out = node(batch.x_dict, batch.edge_index_dict, batch) if kind == "hscn" else node(batch)
    out.square().mean().backward()
    for (name, p), (_, q) in zip(link.named_parameters(), node.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), name
    reached = [n for n, p in link.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0]
    assert any("lin_2" in n or "conv_layers.2" in n for n in reached) and len(reached) >= 4

    # the op a link-level model adds, on its own embedding: dL/dz against float64
    store = _store(kind, batch)
    z = batching.link_forward(link, batch)[2].clone().requires_grad_(True)
    s = pair_dot(z, store.edge_label_index, PairStructure.of(store))
    l, _ = criterion("cross_entropy", s, labels)
    l.backward()
    z64 = z.detach().cpu().double().requires_grad_(True)
    u, v = store.edge_label_index.cpu()
    y = labels.cpu().double()
    s64 = (z64[u] * z64[v]).sum(1)
    l64 = F.binary_cross_entropy_with_logits(s64, y)
    l64.backward()
    P, N = y.numel(), z64.size(0)
    zd = z64.detach()
    g = (torch.sigmoid(s64.detach()) - y) / P
    A = (zd[u].abs() * zd[v].abs()).sum(1)
    G = (D * A / 4 + 4) / P
    deg = torch.bincount(u, minlength=N) + torch.bincount(v, minlength=N)
    first = torch.zeros(N, D, dtype=torch.float64)
    first.index_add_(0, u, g.abs()[:, None] * zd[v].abs())
    first.index_add_(0, v, g.abs()[:, None] * zd[u].abs())
    second = torch.zeros(N, D, dtype=torch.float64)
    second.index_add_(0, u, G[:, None] * zd[v].abs())
    second.index_add_(0, v, G[:, None] * zd[u].abs())
    mag = (deg + 1)[:, None] * first + second
    size = g.abs() * zd[v].abs().max(1).values
    p = int(size.argmax())
    dropped = z64.grad.clone()
    dropped[u[p]] -= g[p] * zd[v[p]]
    check_f64(z.grad, z64.grad, mag, 1, dropped, what=f"{kind} dL/dz")


def _all_pairs_by_pair_dot(zg):
    """[n, n] scores of a graph's rows through the pair decoder itself: the kernel's own float32 values."""
    from graph_hscn.nn.head import pair_dot
    n = zg.size(0)
    a = torch.arange(n, device=DEV)
    pairs = torch.stack([a.repeat_interleave(n), a.repeat(n)])
    return pair_dot(zg.to(DEV).contiguous(), pairs).view(n, n).cpu()


@pytest.mark.parametrize("kind", ["hscn", "mpnn"])
def test_train_runs_a_link_level_model_and_reports_the_per_graph_mrr(kind):
    from graph_hscn.data import DataLoader
    from graph_hscn.metrics import link_means, link_rank_counts
    from graph_hscn.train import batching
    from graph_hscn.train.train import eval_epoch, train
    data = _data(kind, 8, seed=2)
    model = _model(kind, "link")
    loaders = [DataLoader(data, 4, shuffle=False), DataLoader(data[:4], 4, shuffle=False),
               DataLoader(data[4:], 4, shuffle=False)]
    cfg = SimpleNamespace(epochs=2, eval_period=1, loss_fn="cross_entropy", metric="mrr", patience=10, min_delta=0.0)
    opt = SimpleNamespace(optim_type="adam", lr=1e-2, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    history = train(None, opt, cfg, loaders, model)
    assert len(history) == 2 and all(np.isfinite(l) and 0.0 < p <= 1.0 for l, p in history)
    reported = {name: eval_epoch(1, None, loaders[0], model, "cross_entropy", None, "Test", link_metric=name)[1]
                for name in ("mrr", "hits@1", "hits@3", "hits@10")}
    assert reported["mrr"] == eval_epoch(1, None, loaders[0], model, "cross_entropy", None, "Test")[1]
    with pytest.raises(ValueError, match="link_metric="):
        eval_epoch(1, None, loaders[0], model, "cross_entropy", lambda t, s: 0.0, "Test")
    # the same numbers from embeddings recomputed with the final weights (eval mode, no dropout), ranked on the CPU
    model.eval()
    tables, P = [], 0
    with torch.no_grad():
        for batch in loaders[0]:
            batch = batching.to_device(model, batch, DEV)
            z = _embed(kind, model, batch).cpu()
            st = _store(kind, batch)
            tables.append(link_rank_counts(z, st.ptr.cpu(), st.pair_ptr32.cpu(), st.edge_label_index.cpu(),
                                           st.edge_label.cpu(), 1, score=_all_pairs_by_pair_dot)[1])
            P += int(st.edge_label.numel())
    want = link_means(torch.cat(tables), "graph")
    for k, name in enumerate(("mrr", "hits@1", "hits@3", "hits@10")):
        assert abs(reported[name] - want[k]) <= P * EPS64 * want[k], f"{name}: {reported[name]} vs {want[k]}"
