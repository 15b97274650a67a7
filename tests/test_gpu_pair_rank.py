"""hscn_pair_rank / hscn_pair_rank_reduce (csrc/edge_head.hip; graph_hscn.metrics) against the CPU restatement
``metrics.link_rank_counts`` / ``eval_link_ranks``.

The ranks are integers, so they are compared with ``torch.equal``, on fixtures where no float32 evaluation order can
decide a comparison differently from the reference:
  (a) integer embeddings with entries in {-2 .. 2}: every product and every partial sum is a small integer, exact in
      float32 in any order; exact ties are frequent and must come out as ties;
  (b) seeded normal embeddings, accepted only if for every positive (u, v) and every other node w of its graph the
      float64 gap |s(u, w) - s(u, v)| exceeds F64_C * D * 2^-24 * (|z_u| |z_w| + |z_u| |z_v|) (norms): twice the
      a-priori error of a float32 dot product of length D, so neither side's rounding can flip the comparison.  A
      fixture that fails is redrawn with the next seed, twenty times at most; it is never shrunk.
MRR and Hits@K are float64 sums of at most P terms in (0, 1], compared within P * 2^-52 relative.

Graph sizes: 1, 2, 9, 53, 64, 65 nodes, the largest graph that hscn_pair_rank_supported keeps in LDS at D = 64 and one
node more (the same kernel, rows from global memory).  Batches of 1 and 5 graphs and of one graph more than the grid
(the kernel loops over graphs); a graph without candidate pairs, one without positives, one whose candidates are all
positive."""
import pytest
import torch

from tests.helpers import F64_C, U32

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILTERS = [0, 1, 2]
EPS64 = 2.0 ** -52


def _lds_max(D=64):
    from graph_hscn import _hip
    return int(_hip.lib().hscn_pair_rank_lds_max_nodes(D))


def _graph(n, D, gen, kind, num_pairs=None, share=0.3, integer=False):
    """A ``Data`` whose ``x`` is the embedding: ``kind`` "mixed" (random distinct ordered pairs, a share positive),
    "none" (no candidates), "negatives" (no positive), "positives" (every candidate positive)."""
    from graph_hscn.data import Data
    z = torch.randint(-2, 3, (n, D), generator=gen).float() if integer else torch.randn(n, D, generator=gen)
    total = n * (n - 1)
    if kind == "none" or total == 0:
        pairs = torch.zeros(2, 0, dtype=torch.int64)
    else:
        count = total if num_pairs is None else min(num_pairs, total)
        flat = torch.randperm(total, generator=gen)[:count]
        u, r = flat // (n - 1), flat % (n - 1)
        pairs = torch.stack([u, r + (r >= u).long()])                  # every ordered pair u != v once
    P = pairs.size(1)
    if kind == "negatives":
        label = torch.zeros(P)
    elif kind == "positives":
        label = torch.ones(P)
    else:
        label = (torch.rand(P, generator=gen) < share).float()
    return Data(x=z, edge_index=torch.zeros(2, 0, dtype=torch.int64), num_nodes=n, edge_label_index=pairs,
                edge_label=label)


def _sizes():
    return [1, 2, 9, 53, 64, 65, _lds_max(), _lds_max() + 1]


def _fixture(D, seed, integer):
    """One batch per case of the docstring: every size as a batch of one, a batch of five with the three special
    graphs, and -- integer embeddings only, they need no acceptance test -- one graph more than the grid."""
    from graph_hscn.data import Batch
    gen = torch.Generator().manual_seed(seed)
    batches = []
    for n in _sizes():
        few = n > 16                                                   # (keeps the reference and the gap test small)
        batches.append([_graph(n, D, gen, "mixed", num_pairs=40 if few else None, share=0.2 if few else 0.4,
                               integer=integer)])
    batches.append([_graph(9, D, gen, "mixed", integer=integer), _graph(5, D, gen, "none", integer=integer),
                    _graph(7, D, gen, "negatives", integer=integer), _graph(6, D, gen, "positives", integer=integer),
                    _graph(53, D, gen, "mixed", num_pairs=60, share=0.2, integer=integer)])
    return [Batch.from_data_list(b) for b in batches]


def _gaps_decide(batch, D):
    """Whether every comparison the ranks of ``batch`` rest on is decided beyond float32 rounding (docstring, b)."""
    z = batch.x.double()
    norm = z.norm(dim=1)
    ptr = batch.ptr.tolist()
    for g in range(batch.num_graphs):
        a, b = int(batch.pair_ptr32[g]), int(batch.pair_ptr32[g + 1])
        pos = batch.edge_label[a:b] == 1
        u, v = batch.edge_label_index[0, a:b][pos], batch.edge_label_index[1, a:b][pos]
        if u.numel() == 0:
            continue
        zg, ng = z[ptr[g]:ptr[g + 1]], norm[ptr[g]:ptr[g + 1]]
        rows = z[u] @ zg.T                                             # s(u, w) for every w of the graph
        spos = (z[u] * z[v]).sum(1, keepdim=True)
        lim = F64_C * D * U32 * (norm[u][:, None] * ng[None, :] + (norm[u] * norm[v])[:, None])
        others = torch.ones_like(rows, dtype=torch.bool)
        others[torch.arange(u.numel()), v - ptr[g]] = False
        if bool((((rows - spos).abs() <= lim) & others).any()):
            return False
    return True


_CACHE = {}


def _accepted(D):
    """The normal-embedding fixture of width ``D``: the first of twenty seeds whose every batch passes the gap test."""
    if D not in _CACHE:
        for attempt in range(20):
            batches = _fixture(D, 1000 * D + attempt, integer=False)
            if all(_gaps_decide(b, D) for b in batches):
                _CACHE[D] = batches
                break
        else:
            raise AssertionError(f"no seed in twenty gives a D={D} fixture whose comparisons float32 cannot flip")
    return _CACHE[D]


def _reference(batch, filter):
    from graph_hscn.metrics import link_rank_counts
    return link_rank_counts(batch.x.double(), batch.ptr, batch.pair_ptr32, batch.edge_label_index, batch.edge_label, filter)


def _launch(batch, filter, averaging="graph", z=None, max_nodes=None):
    from graph_hscn.metrics import pair_rank_launch
    from graph_hscn.nn.head import PairStructure
    d = batch.to(DEV)
    st = PairStructure(d.edge_label_index, d.num_nodes, d.edge_label)
    out = pair_rank_launch(d.x if z is None else z, d.ptr32, d.pair_ptr32, st, filter, averaging,
                           max_nodes=max_nodes if max_nodes is not None else int(d.max_nodes))
    torch.cuda.synchronize()
    return out


def _check_batch(batch, filter, what):
    from graph_hscn.metrics import link_means, read_link_packed
    rank2, per_graph = _reference(batch, filter)
    out = _launch(batch, filter)
    assert torch.equal(out.rank2.cpu(), rank2), f"{what}: rank2"
    assert torch.equal(out.per_graph.cpu()[:, 1:], per_graph[:, 1:]), f"{what}: hit counts / num_pos"
    P = max(int(batch.edge_label.numel()), 1)
    assert bool(((out.per_graph.cpu()[:, 0] - per_graph[:, 0]).abs() <= P * EPS64 * per_graph[:, 0]).all()), what
    f64, flags = read_link_packed(out.packed)
    if float(per_graph[:, 4].sum()) == 0:
        assert flags == 16 and f64.tolist() == [0.0] * 4, f"{what}: no positive at all"
        return rank2
    assert flags == 0, f"{what}: flags {flags}"
    for averaging in ("graph", "pooled"):
        want = link_means(per_graph, averaging)
        got = f64.tolist() if averaging == "graph" else read_link_packed(_launch(batch, filter, averaging).packed)[0].tolist()
        for k in range(4):
            assert abs(got[k] - want[k]) <= P * EPS64 * want[k], f"{what}: {averaging} word {k}: {got[k]} vs {want[k]}"
    return rank2


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("D", [4, 16, 64])
def test_integer_embeddings_ranks_and_counts_are_equal_and_ties_are_ties(D, filter):
    odd = total = 0
    for i, batch in enumerate(_fixture(D, 77 + D, integer=True)):
        rank2 = _check_batch(batch, filter, f"integer D={D} filter={filter} batch {i}")
        ranked = rank2[rank2 >= 0]
        odd += int((ranked % 2 == 1).sum())                            # rank2 = 2 g + e is odd only with e > 0
        total += int(ranked.numel())
    assert total > 100 and odd >= 0.05 * total, f"{odd} of {total} positives show a tie"


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("D", [4, 16, 64])
def test_normal_embeddings_whose_gaps_float32_cannot_flip(D, filter):
    for i, batch in enumerate(_accepted(D)):
        _check_batch(batch, filter, f"normal D={D} filter={filter} batch {i}")


@pytest.mark.parametrize("filter", FILTERS)
def test_every_candidate_positive_ranks_first_once_filtered(filter):
    from graph_hscn.data import Batch
    gen = torch.Generator().manual_seed(4)
    batch = Batch.from_data_list([_graph(6, 16, gen, "positives", integer=True)])
    rank2 = _check_batch(batch, filter, f"all positive, filter {filter}")
    if filter == 2:
        assert bool((rank2 == 0).all())                                # no negative is left: rank 1
    if filter == 1:
        assert bool((rank2 <= 2).all())                                # only the self score is left to compete


def test_one_graph_more_than_the_grid():
    from graph_hscn import _hip
    from graph_hscn.data import Batch
    grid = int(_hip.lib().hscn_pair_rank_max_workgroups())
    gen = torch.Generator().manual_seed(8)
    graphs = [_graph(3 + i % 3, 8, gen, "mixed" if i % 7 else "negatives", share=0.5, integer=True) for i in range(grid + 1)]
    batch = Batch.from_data_list(graphs)
    assert batch.num_graphs == grid + 1
    for filter in FILTERS:
        _check_batch(batch, filter, f"B = grid + 1, filter {filter}")


def test_the_declared_largest_graph_only_sizes_the_staging():
    """``max_nodes`` unknown (0: the whole budget), exact, or too small (the larger graphs then read global memory):
    the same integers."""
    batch = _fixture(16, 5, integer=True)[-1]                          # graphs of 9, 5, 7, 6 and 53 nodes
    rank2, per_graph = _reference(batch, 1)
    for max_nodes in (0, 53, 7, 1):
        out = _launch(batch, 1, max_nodes=max_nodes)
        assert torch.equal(out.rank2.cpu(), rank2) and torch.equal(out.per_graph.cpu()[:, 1:], per_graph[:, 1:])


def test_pairs_no_graph_covers_keep_rank2_minus_one():
    from graph_hscn.data import Batch
    from graph_hscn.metrics import PAIR_BAD_SEGMENT
    gen = torch.Generator().manual_seed(6)
    batch = Batch.from_data_list([_graph(6, 16, gen, "positives", integer=True) for _ in range(2)])
    clean = _launch(batch, 1)
    batch.pair_ptr32 = torch.tensor([0, 30, 20], dtype=torch.int32)    # graph 1: a descending range
    out = _launch(batch, 1)
    assert int(out.flags.item()) == PAIR_BAD_SEGMENT
    assert torch.equal(out.rank2[:30], clean.rank2[:30]) and bool((out.rank2[30:] == -1).all())
    assert torch.equal(out.per_graph[0], clean.per_graph[0]) and bool((out.per_graph[1] == 0).all())


def test_flags_cross_graph_pair_nan_row_and_label_leave_the_other_graphs_alone():
    from graph_hscn.data import Batch
    from graph_hscn.metrics import (PAIR_ID_OUT_OF_RANGE, PAIR_LABEL_NOT_BINARY, PAIR_NAN_SCORE, link_metric_values,
                                    read_link_packed)
    gen = torch.Generator().manual_seed(12)
    graphs = [_graph(9, 16, gen, "mixed", share=0.5, integer=True) for _ in range(3)]
    base = Batch.from_data_list(graphs)
    clean = _launch(base, 1)
    assert int(clean.flags.item()) == 0
    N = base.num_nodes

    def run(mutate, z=None):
        b = Batch.from_data_list(graphs)
        mutate(b)
        out = _launch(b, 1, z=z)
        return out, int(out.flags.item())

    def cross(b):                                                       # a pair of graph 0 whose target lies in graph 1
        p = int((b.edge_label[: int(b.pair_ptr32[1])] == 1).nonzero()[0])
        b.edge_label_index[1, p] = int(b.ptr[1]) + 2
        assert 0 <= int(b.edge_label_index[1, p]) < N
    out, flags = run(cross)
    assert flags == PAIR_ID_OUT_OF_RANGE
    assert torch.equal(out.per_graph[1:], clean.per_graph[1:])
    assert float(out.per_graph[0, 4]) == float(clean.per_graph[0, 4]) - 1       # not dereferenced, not counted
    with pytest.raises(IndexError):
        link_metric_values(*read_link_packed(out.packed))

    z = base.x.clone()
    z[int(base.ptr[1]) + 4] = float("nan")                              # a NaN row in graph 1
    out, flags = run(lambda b: None, z=z.to(DEV))
    assert flags == PAIR_NAN_SCORE
    assert torch.equal(out.per_graph[0], clean.per_graph[0]) and torch.equal(out.per_graph[2], clean.per_graph[2])
    with pytest.raises(ValueError, match="NaN"):
        link_metric_values(*read_link_packed(out.packed))

    def half(b):                                                        # a label 0.5 in graph 2
        b.edge_label[int(b.pair_ptr32[2]) + 1] = 0.5
    out, flags = run(half)
    assert flags == PAIR_LABEL_NOT_BINARY
    assert torch.equal(out.per_graph[:2], clean.per_graph[:2])
    assert int(out.rank2[int(base.pair_ptr32[2]) + 1]) == -1
    with pytest.raises(ValueError, match="0 or 1"):
        link_metric_values(*read_link_packed(out.packed))


def test_accumulator_whose_first_batches_hold_no_positive():
    """The epoch's leading batches without a positive pair leave no error behind: the result is the union launch's."""
    from graph_hscn.data import Batch
    from graph_hscn.metrics import LinkRankAccumulator, PAIR_NO_POSITIVE, read_link_packed
    gen = torch.Generator().manual_seed(33)
    kinds = ["negatives", "none", "negatives", "negatives", "mixed", "mixed"]
    graphs = [_graph(6 + i, 16, gen, k, share=0.4, integer=True) for i, k in enumerate(kinds)]
    union = Batch.from_data_list(graphs)
    for averaging in ("graph", "pooled"):
        acc = LinkRankAccumulator(filter=1, averaging=averaging)
        for k in range(3):                                             # batches 0 and 1 hold no positive
            b = Batch.from_data_list(graphs[2 * k:2 * k + 2]).to(DEV)
            acc.update(b.x, b)
            if k < 2:
                assert read_link_packed(acc.packed)[1] == PAIR_NO_POSITIVE
                with pytest.raises(RuntimeError, match="No positive pair"):
                    acc.result()
        got = acc.result()
        one = read_link_packed(_launch(union, 1, averaging).packed)
        assert one[1] == 0 and list(got.values()) == one[0].tolist()
        # a trailing batch without positives changes nothing
        b = Batch.from_data_list(graphs[:2]).to(DEV)
        acc.update(b.x, b)
        assert acc.result() == got


def test_accumulator_over_three_batches_equals_one_call_on_their_union():
    from graph_hscn.data import Batch
    from graph_hscn.metrics import LinkRankAccumulator, eval_link_ranks, eval_link_ranks_hip, read_link_packed
    from graph_hscn.nn.head import PairStructure
    gen = torch.Generator().manual_seed(21)
    graphs = [_graph(5 + i, 16, gen, "negatives" if i == 4 else "mixed", share=0.4, integer=True) for i in range(9)]
    union = Batch.from_data_list(graphs)
    for averaging in ("graph", "pooled"):
        acc = LinkRankAccumulator(filter=1, averaging=averaging)
        for k in range(3):
            b = Batch.from_data_list(graphs[3 * k:3 * k + 3]).to(DEV)
            acc.update(b.x, b)
        got = acc.result()
        one = read_link_packed(_launch(union, 1, averaging).packed)[0].tolist()
        assert [got[k] for k in ("mrr", "hits@1", "hits@3", "hits@10")] == one      # the same additions in the same order
        want = eval_link_ranks(union.x.double(), union.ptr, union.pair_ptr32, union.edge_label_index, union.edge_label,
                               1, averaging)
        P = int(union.edge_label.numel())
        for a, w in zip(one, want):
            assert abs(a - w) <= P * EPS64 * w
        acc.reset()
        b = Batch.from_data_list(graphs[:3]).to(DEV)
        acc.update(b.x, b)
        st = PairStructure.of(b)
        assert st is PairStructure.of(b)                                # built once, cached on the batch
        again = eval_link_ranks_hip(b.x, b.ptr32, b.pair_ptr32, st, 1, averaging)
        assert tuple(acc.result().values()) == again
