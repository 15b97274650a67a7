"""DMoN pooling on the device (csrc/dmon.hip, nn.pool.dmon_pool_sparse, SCN(pool="dmon"), train_clustering) against
the plain-torch restatement tests/dmon_oracle.py under the float64 referee (tests/helpers.py), with the bar's teeth;
determinism; the LDS opt-in line and the LDS refusal; the edgeless graph; the model level."""
import copy

import pytest
import torch

from graph_hscn import _hip
from graph_hscn._hip import ptr, stream
from graph_hscn.nn.functional import DMON_STATS, DMoNSparseFn
from graph_hscn.structure import Relation
from tests import dmon_oracle as DO
from tests.helpers import DEV, check_f64, drop_largest_product, f64_close, referee_all

pytestmark = pytest.mark.gpu


def _device_inputs(graphs):
    logits, x, ei, sizes = DO.flat(graphs)
    N = sum(sizes)
    rel = Relation(ei.to(DEV), N, N)
    nptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    return logits.to(DEV), (x.to(DEV) if x is not None else None), rel, nptr, len(sizes)


def _raw(graphs, weights=DO.WEIGHTS):
    """hscn_dmon_sparse_fwd + _bwd called directly: every buffer of the C ABI, on the host."""
    lg, x, rel, nptr, G = _device_inputs(graphs)
    N, K = lg.shape
    Fx = x.shape[1] if x is not None else 0
    new = lambda *s: torch.full(s, float("nan"), device=DEV)       # noqa: E731  (a cell the kernel skips stays NaN)
    out = dict(S=new(N, K), stats=new(G, DMON_STATS), ss=new(G, K, K), vec=new(G, 2, K), pooled_adj=new(G, K, K),
               losses=new(3), g_logits=new(N, K), pooled_x=new(G, K, Fx) if Fx else None)
    r, c = rel.csr_t, rel.csr
    _hip.call("hscn_dmon_sparse_fwd", ptr(lg), ptr(x), ptr(r.rowptr), ptr(r.col), ptr(nptr), ptr(out["S"]),
              ptr(out["stats"]), ptr(out["ss"]), ptr(out["vec"]), ptr(out["pooled_x"]), ptr(out["pooled_adj"]),
              ptr(out["losses"]), N, G, K, Fx, stream())
    gl = torch.tensor(weights, dtype=torch.float32, device=DEV)
    _hip.call("hscn_dmon_sparse_bwd", ptr(out["S"]), ptr(out["stats"]), ptr(out["ss"]), ptr(out["vec"]), ptr(r.rowptr),
              ptr(r.col), ptr(c.rowptr), ptr(c.col), ptr(nptr), ptr(gl), ptr(out["g_logits"]), N, G, K, stream())
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def _through_autograd(graphs, weights=DO.WEIGHTS):
    lg, x, rel, nptr, G = _device_inputs(graphs)
    lg.requires_grad_()
    S, sp, o, cl, px, padj = DMoNSparseFn.apply(lg, x, rel, nptr, G)
    (weights[0] * sp + weights[1] * o + weights[2] * cl).backward()
    return dict(S=S.cpu(), losses=torch.stack([sp, o, cl]).detach().cpu(), pooled_x=px.cpu() if px is not None else None,
                pooled_adj=padj.cpu(), g_logits=lg.grad.cpu())


def _got(raw):
    """What ``dmon_oracle.referee_case`` compares, from the kernel's buffers (the spectral loss's two terms from the
    statistics row: include/hscn.h)."""
    st = raw["stats"].double()
    tm = torch.where(st[:, 1] > 0, st[:, 1], torch.ones_like(st[:, 1]))
    return {"spectral": raw["losses"][0:1], "ortho": raw["losses"][1:2], "cluster": raw["losses"][2:3],
            "trace/2m": st[:, 0] / tm, "null/2m": st[:, 2] / tm, "g_logits": raw["g_logits"]}


def _check_statistics_row(raw, graphs):
    """The row's remaining cells (2m exact; |S^T S|, ortho_g, |c|, the per-graph losses) and ss / vec against float64:
    sums of <= n + K^2 non-negative terms (mag = the value), the spectral cell at its larger term's size."""
    f = DO.forward(graphs)
    st, n_max, K = raw["stats"], max(lg.size(0) for lg, _, _ in graphs), graphs[0][0].size(1)
    depth = n_max + K * K + 32
    assert torch.equal(st[:, 1].double(), f["two_m"])
    assert f64_close(st[:, 3], f["ss_norm"], f["ss_norm"], depth, what="|S^T S|")
    assert f64_close(st[:, 4], f["ortho_g"], 1.0, depth, what="ortho_g")
    assert f64_close(st[:, 5], f["c_norm"], f["c_norm"], depth, what="|c|")
    tm = torch.where(f["two_m"] > 0, f["two_m"], torch.ones_like(f["two_m"]))
    assert f64_close(st[:, 6], f["spectral_g"], torch.maximum(f["trace"], f["null"]) / tm, 2 * n_max + 2 * K + 32,
                     what="spectral_g")
    assert f64_close(st[:, 7], f["cluster_g"], f["cluster_g"].abs() + 1.0, depth, what="cluster_g")
    assert f64_close(raw["ss"], f["ss"], f["ss"], n_max + 8, what="ss")
    deg = max(int(torch.bincount(ei[0]).max()) if ei.numel() else 0 for _, _, ei in graphs)
    assert f64_close(raw["vec"], f["vec"], f["vec"], n_max + 8, what="vec")
    return f, deg


def _check_pooled(raw, graphs, f, deg):
    """pooled_x = selu(S^T X) and pooled_adj against float64 with a-priori magnitudes, each with its teeth: the largest
    product left out of one element of S^T X, one edge left out of the largest graph's adjacency."""
    K = graphs[0][0].size(1)
    S64 = torch.softmax(torch.cat([lg for lg, _, _ in graphs]).double(), 1)
    selu = torch.nn.functional.selu
    off = 0
    for b, (lg, x, ei) in enumerate(graphs):
        n = lg.size(0)
        Sb = S64[off:off + n]
        off += n
        if x.size(1):
            xb = x.double()
            pre = Sb.t() @ xb
            dropped = drop_largest_product(f["pooled_x"][b], Sb.t(), xb,
                                           post=lambda r, o, t, pre=pre: float(selu(pre[r, o] - t)))
            # selu is 1.0507-Lipschitz up to its own rounding: the pre-activation's bound, plus a few ulp of |y|
            check_f64(raw["pooled_x"][b], f["pooled_x"][b], 1.06 * (Sb.t() @ xb.abs()) + f["pooled_x"][b].abs(), n + 12,
                      dropped, what=f"pooled x graph {b}")
        # S^T A S: sums of n (deg + 1) non-negative terms, then two divisions by roots of row sums of K of them
        depth = n + deg + K + 16
        assert f64_close(raw["pooled_adj"][b], f["pooled_adj"][b], f["pooled_adj"][b], depth, what=f"pooled adj graph {b}")
    if K > 1:
        b = max(range(len(graphs)), key=lambda i: graphs[i][0].size(0))
        short = DO.forward(graphs, drop_edge=(b, 0))["pooled_adj"][b]
        n = graphs[b][0].size(0)
        assert not f64_close(raw["pooled_adj"][b], short, f["pooled_adj"][b], n + deg + K + 16), \
            "the pooled-adjacency bound cannot see a dropped edge"


def _check_S(raw, graphs):
    K = graphs[0][0].size(1)
    l64 = torch.cat([lg for lg, _, _ in graphs]).double()
    S64 = torch.softmax(l64, 1)
    spread = float((l64 - l64.max(1, keepdim=True).values).abs().max())
    assert f64_close(raw["S"], S64, S64, K + 8 + spread, tiny=1e-37, what="S")


@pytest.mark.parametrize("Fx", [0, 7], ids=["fx0", "fx7"])
@pytest.mark.parametrize("K", [1, 2, 5, 64])
def test_operator_against_the_float64_referee(K, Fx):
    """Graphs of 1, 2, 37, 100 and 130 nodes in one batch (a single node, off-tile, more than one tile pass), self loops,
    a duplicated and a one-directional edge per graph beyond 3 nodes; logits N(0, 2^2); loss mix 1.3 spectral +
    0.7 ortho + 0.9 cluster.  The bar is ``dmon_oracle.referee_case`` (eight relabelled float32 oracle draws, the
    spectral loss at its larger term's scale and its two terms separately from the statistics row; teeth: the null
    model, the A^T half, the cluster term).  tests/test_dmon_host.py tries the same bar on a ninth float32 draw:
    ratios 0.09 .. 0.40 there."""
    graphs = DO.case(K, Fx)
    raw = _raw(graphs)
    assert all(bool(torch.isfinite(v).all()) for v in raw.values() if v is not None)
    worst = DO.referee_case(_got(raw), graphs, f"dmon K={K} Fx={Fx}")
    print(f"   worst referee ratio K={K} Fx={Fx}: {worst:.3f}")
    _check_S(raw, graphs)
    f, deg = _check_statistics_row(raw, graphs)
    _check_pooled(raw, graphs, f, deg)
    # the autograd function is those two calls: the same bits
    auto = _through_autograd(graphs)
    for k, v in auto.items():
        if v is None:
            assert raw[k] is None
        elif k == "pooled_x":
            assert torch.equal(v[:, :, :Fx], raw[k]), k
        else:
            assert torch.equal(v, raw[k]), k


def test_same_call_twice_and_a_graph_alone_or_last_in_a_batch():
    """Run to run every output is bit-equal.  A graph alone and as the last of five: its S rows, statistics row and ss
    block are bit-equal (one workgroup per graph, sums in node order).  Its g_logits rows carry the factor 1 / G of the
    mean over graphs: compared as the last of EIGHT, where the factor is a power of two and every product by it exact,
    so G * row is bit-equal to the row of the graph alone."""
    K = 5
    five = DO.case(K, 7)
    a, b = _raw(five), _raw(five)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    alone = _raw(five[-1:])
    n = five[-1][0].size(0)
    assert torch.equal(alone["S"], a["S"][-n:])
    assert torch.equal(alone["stats"][0], a["stats"][-1])
    assert torch.equal(alone["ss"][0], a["ss"][-1]) and torch.equal(alone["vec"][0], a["vec"][-1])
    assert torch.equal(alone["pooled_x"][0], a["pooled_x"][-1]) and torch.equal(alone["pooled_adj"][0], a["pooled_adj"][-1])
    eight = DO.case(K, 7, sizes=[3, 9, 16])[:3] + five
    e = _raw(eight)
    assert torch.equal(alone["stats"][0], e["stats"][-1])
    assert float(alone["g_logits"].abs().max()) > 0
    assert torch.equal(alone["g_logits"], 8.0 * e["g_logits"][-n:])


@pytest.mark.parametrize("K", [82, 83, 112, 113])
def test_at_the_lds_opt_in_line(K):
    """Without x, k_dmon_stats asks for (2 K^2 + 35 K + 20) * 4 bytes of LDS (two K x K accumulators, two 16 x K tiles,
    16 degrees, the K-vectors d^T S, c and the pooled-adjacency row norms, 4 spare) and k_dmon_bwd for
    (K^2 + 34 K + 20) * 4 (one K x K, two tiles, two K-vectors, 16 row dots, 4 spare): K = 82 is the last width whose forward stays within the
    64 KB a launch gets unasked (65352 bytes) and 83 the first that opts in (66812); 112 (65488) / 113 (66524) are the
    same pair for the backward.  Two small graphs; the bar of test_operator_against_the_float64_referee."""
    assert (2 * 82 * 82 + 35 * 82 + 20) * 4 <= 65536 < (2 * 83 * 83 + 35 * 83 + 20) * 4
    assert (112 * 112 + 34 * 112 + 20) * 4 <= 65536 < (113 * 113 + 34 * 113 + 20) * 4
    graphs = DO.case(K, 0, sizes=[5, 20])
    raw = _raw(graphs)
    DO.referee_case(_got(raw), graphs, f"dmon K={K}")
    _check_S(raw, graphs)
    _check_statistics_row(raw, graphs)


def test_k256_is_unsupported():
    """K = 256 passes the argument check; its K x K accumulators exceed a CU's 160 KB in both directions."""
    graphs = DO.case(256, 0, sizes=[5])
    lg, _, rel, nptr, G = _device_inputs(graphs)
    K = 256
    S, stats, ss = torch.empty_like(lg), torch.empty(1, DMON_STATS, device=DEV), torch.empty(1, K, K, device=DEV)
    vec, losses, gl = torch.empty(1, 2, K, device=DEV), torch.empty(3, device=DEV), torch.ones(3, device=DEV)
    r, c = rel.csr_t, rel.csr
    lib = _hip.lib()
    assert lib.hscn_dmon_sparse_fwd(ptr(lg), None, ptr(r.rowptr), ptr(r.col), ptr(nptr), ptr(S), ptr(stats), ptr(ss),
                                    ptr(vec), None, None, ptr(losses), 5, 1, K, 0, stream()) == -3
    assert lib.hscn_dmon_sparse_bwd(ptr(S), ptr(stats), ptr(ss), ptr(vec), ptr(r.rowptr), ptr(r.col), ptr(c.rowptr),
                                    ptr(c.col), ptr(nptr), ptr(gl), ptr(torch.empty_like(lg)), 5, 1, K, stream()) == -3
    with pytest.raises(RuntimeError):
        DMoNSparseFn.apply(lg, None, rel, nptr, 1)
    torch.cuda.synchronize()


def test_edgeless_graph_in_a_batch_of_three():
    """2m = 0 (no self loops either: operator level only): spectral_g = 0 and no spectral gradient, nothing NaN."""
    K = 4
    graphs = DO.case(K, 3, sizes=[9, 6, 20])
    lone = (graphs[1][0], graphs[1][1], torch.zeros(2, 0, dtype=torch.long))
    graphs = [graphs[0], lone, graphs[2]]
    raw = _raw(graphs)
    assert all(bool(torch.isfinite(v).all()) for v in raw.values() if v is not None)
    assert float(raw["stats"][1, 1]) == 0.0 and float(raw["stats"][1, 2]) == 0.0 and float(raw["stats"][1, 6]) == 0.0
    only_spectral = _raw(graphs, weights=(1.0, 0.0, 0.0))["g_logits"]
    assert float(only_spectral[9:15].abs().max()) == 0.0
    assert float(only_spectral[:9].abs().max()) > 0 and float(only_spectral[15:].abs().max()) > 0
    f64 = DO.forward(graphs)
    for i, k in enumerate(("spectral", "ortho", "cluster")):
        assert abs(float(raw["losses"][i]) - float(f64[k])) <= 1e-5, k
    g64 = DO.backward(graphs)
    assert float((raw["g_logits"].double() - g64).abs().max()) <= 1e-5 * max(1.0, float(g64.abs().max()))


# --------------------------------------------------------------------------- #
# model level
# --------------------------------------------------------------------------- #
def _planted(num, seed, cliques=4, feat=9):
    """``num`` small graphs of ``cliques`` cliques (3 .. 6 nodes each) chained by single edges; features = noise plus
    a one-hot of the clique in the first columns."""
    from graph_hscn.data import Data
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(num):
        sizes = torch.randint(3, 7, (cliques,), generator=g).tolist()
        member = torch.cat([torch.full((s,), c) for c, s in enumerate(sizes)])
        n = member.numel()
        same = (member.unsqueeze(0) == member.unsqueeze(1)) & ~torch.eye(n, dtype=torch.bool)
        src, dst = same.nonzero(as_tuple=True)
        firsts = torch.tensor([0] + torch.tensor(sizes).cumsum(0)[:-1].tolist())
        bridge = torch.stack([torch.cat([firsts[:-1], firsts[1:]]), torch.cat([firsts[1:], firsts[:-1]])])
        x = 0.3 * torch.randn(n, feat, generator=g)
        x[torch.arange(n), member] += 1.0
        out.append(Data(x=x, edge_index=torch.cat([torch.stack([src, dst]), bridge], 1), num_nodes=n))
    return out


def scn_dmon_step_in_dtype(m, graphs):
    """The stage-A body of an ``SCN(pool="dmon")`` on the oracle's modules, in the dtype of ``m``'s parameters: per graph
    gcn_norm(add_self_loops=True) -> message passing -> MLP -> DMoN (tests/dmon_oracle.py) on the normalised edge list,
    weights ignored; losses = mean over the graphs.  Returns (softmax assignment, spectral, ortho, cluster)."""
    from oracle import pyg_ops as P
    dt = m.mp.module_0.lin_rel.weight.dtype
    per_graph = []
    for d in graphs:
        ei2, ew = P.gcn_norm(d.edge_index, None, d.x.size(0), add_self_loops=True, dtype=dt)
        h = m.mp(d.x.to(dt), ei2, ew)
        per_graph.append((m._run_mlp(h), h.detach(), ei2))
    f = DO.forward(per_graph, dt)
    return f["S"], f["spectral"], f["ortho"], f["cluster"]


def test_scn_dmon_step_against_an_oracle_twin():
    """One forward_graphs + backward of SCN([16], "relu", 9, 4, pool="dmon") on a three-graph batch: S, the three
    losses and every parameter gradient inside the referee against the oracle twin (float32 and float64 from the same
    weights)."""
    from graph_hscn.data import Batch
    from graph_hscn.model.hscn import SCN
    from oracle import models as OM
    torch.manual_seed(11)
    graphs = _planted(3, seed=2)
    om = OM.SCN([16], "relu", 9, 4)
    pm = SCN([16], "relu", 9, 4, pool="dmon").to(DEV)
    pm.load_state_dict(om.state_dict())
    res = {}
    for dt in (torch.float32, torch.float64):
        m = copy.deepcopy(om).to(dt)
        S, sp, o, cl = scn_dmon_step_in_dtype(m, graphs)
        (sp + o + cl).backward()
        res[dt] = {"S": S.detach(), "spectral": sp.detach().reshape(1), "ortho": o.detach().reshape(1),
                   "cluster": cl.detach().reshape(1)}
        res[dt].update({"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()})
    S, sp, o, cl, total = pm.forward_graphs(Batch.from_data_list(graphs), with_total=True)
    assert pm.last_engine == "layered" and pm.last_route == "sparse"
    total.backward()
    got = {"S": S.detach(), "spectral": sp.detach().reshape(1), "ortho": o.detach().reshape(1),
           "cluster": cl.detach().reshape(1)}
    got.update({"p." + n: p.grad.detach().clone() for n, p in pm.named_parameters()})
    assert float(total.detach()) == float((sp + o + cl).detach())
    referee_all(got, res[torch.float32], res[torch.float64], "scn dmon step")
    # the single-graph call returns the five-slot tuple with the dense adjacency, as MinCUT's four-slot one does
    from graph_hscn.nn.pool import gcn_norm
    d = graphs[0]
    ei, ew = gcn_norm(d.edge_index.to(DEV), None, d.num_nodes, add_self_loops=True)
    out = pm(d.x.to(DEV), ei, ew)
    assert len(out) == 5 and out[4].shape == (1, d.num_nodes, d.num_nodes)


def test_dmon_model_is_declined_by_the_one_launch_stage_a_paths():
    from graph_hscn.data import Batch
    from graph_hscn.model.hscn import SCN
    from graph_hscn.step import ScnEpochRunner, ScnTrainStep
    from graph_hscn.train.train_clustering import _train_clustering_direct
    graphs = _planted(3, seed=2)
    pm = SCN([16], "relu", 9, 4, pool="dmon").to(DEV)
    big = Batch.from_data_list(graphs)
    assert pm.resident_ok(big) is False
    assert SCN([16], "relu", 9, 4).to(DEV).resident_ok(big) is True
    assert ScnEpochRunner.eligible(pm, big, "adam") is False
    with pytest.raises(RuntimeError):
        ScnTrainStep(pm, big.to(DEV))
    from graph_hscn.config.config import HSCNConfig, OptimConfig
    assert _train_clustering_direct(None, graphs, pm, HSCNConfig("relu", num_clusters=4, cluster_epochs=1),
                                    OptimConfig("adam", lr=0.01), 1, torch.device(DEV)) is None
    half = Batch.from_data_list(graphs).to(DEV)
    half.x = half.x.half()
    with pytest.raises(RuntimeError, match="half-precision feature storage runs on the fused stage-A launch only"):
        pm.forward_graphs(half)


CLUSTER_LR, CLUSTER_EPOCHS = 0.01, 10


def _oracle_total(state, graphs):
    from oracle import models as OM
    m = OM.SCN([16], "relu", 9, 4).double()
    m.load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    with torch.no_grad():
        return sum(float(sum(scn_dmon_step_in_dtype(m, [d])[1:])) for d in graphs) / len(graphs)


def test_train_clustering_fits_a_dmon_model():
    """Twelve planted-clique graphs, Adam lr 0.01, 10 epochs, one step per graph.  The float64 oracle loop from the same
    initial weights lowers the float64 oracle's total (mean over the graphs of spectral + ortho + cluster) by more than
    10 % (checked here too); the device run must achieve at least half that decrease, measured by the same float64
    oracle at its parameters.  A MinCUT SCN built without the keyword still takes the resident path on the same data."""
    import numpy as np
    from graph_hscn.config.config import HSCNConfig, OptimConfig, TrainingConfig
    from graph_hscn.model.hscn import SCN
    from graph_hscn.train.train_clustering import train_clustering
    from oracle import models as OM
    K = 4
    graphs = _planted(12, seed=4)
    torch.manual_seed(7)
    om = OM.SCN([16], "relu", 9, K)
    pm = SCN([16], "relu", 9, K, pool="dmon").to(DEV)
    pm.load_state_dict(om.state_dict())
    before = _oracle_total(om.state_dict(), graphs)
    o64 = copy.deepcopy(om).double()
    opt = torch.optim.Adam(o64.parameters(), lr=CLUSTER_LR)
    for _ in range(CLUSTER_EPOCHS):
        for d in graphs:
            opt.zero_grad()
            sum(scn_dmon_step_in_dtype(o64, [d])[1:]).backward()
            opt.step()
    oracle_after = _oracle_total(o64.state_dict(), graphs)
    mc = HSCNConfig("relu", num_clusters=K, cluster_epochs=CLUSTER_EPOCHS)
    oc = OptimConfig("adam", lr=CLUSTER_LR)
    tc = TrainingConfig("hscn", "cross_entropy", "ap")
    ids = train_clustering(None, graphs, pm, mc, oc, tc)
    assert pm.last_engine == "layered"
    assert len(ids) == 12
    assert all(c.shape[0] == g.num_nodes and c.dtype == np.int64 and 0 <= c.min() and c.max() < K
               for c, g in zip(ids, graphs))
    after = _oracle_total(pm.state_dict(), graphs)
    print(f"   float64 oracle total: before {before:.6f}, oracle loop {oracle_after:.6f}, device loop {after:.6f}")
    assert before - oracle_after >= 0.10 * abs(before)
    assert before - after >= 0.5 * (before - oracle_after)
    batched = SCN([16], "relu", 9, K, pool="dmon").to(DEV)
    ids_b = train_clustering(None, graphs, batched, HSCNConfig("relu", num_clusters=K, cluster_epochs=1), oc, tc,
                             batch_graphs=5)
    assert batched.last_engine == "layered" and [c.shape[0] for c in ids_b] == [g.num_nodes for g in graphs]
    plain = SCN([16], "relu", 9, K).to(DEV)
    train_clustering(None, graphs, plain, HSCNConfig("relu", num_clusters=K, cluster_epochs=1), oc, tc)
    assert plain.last_engine == "resident" and plain.pool == "mincut"
