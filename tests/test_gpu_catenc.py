"""Categorical encoders on the HIP path (csrc/catenc.hip) against their plain-torch restatement
(``nn.functional.CategoricalEmbedFn``'s CPU branch).

Bars, all from tests/helpers.py, no new constants:
  * the forward and the index build are integer plumbing and ordered adds: ``torch.equal``;
  * the backward (a sum of up to 2 048 cotangent rows per table row) by ``check_f64``: |dW - dW64| <= 3 n 2^-24 mag
    with n = max(count_r, 1) and mag = sum |dOut| over the row; the same bound must REJECT dW64 with the row's
    largest-magnitude term removed;
  * models by ``referee_all`` with ``teeth``: the float32 and float64 CPU runs of the same model are the two oracles
    (oracle GCNConv / the GatedGCN + attention restatements, with the encoders' CPU branch in front); the toothed
    reference leaves one (node, column) term out of an encoder's sum.

Gate condition, as tests/test_gpu_gine.py states it and asserted with no exclusion: every ReLU input of the float64 run
lies farther from zero than 4 x the referee's own limit for its tensor (2 max|f32 - f64| + 8 2^-23 max|f64|).  The
seeds were chosen on the CPU, from the reference alone, so that it holds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from graph_hscn import _hip
from graph_hscn.config.config import ACT_DICT, CONV_DICT, MPNNConfig
from graph_hscn.data import Batch, DataLoader
from graph_hscn.encoder import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS, AtomEncoder, BondEncoder, CategoricalEncoder
from graph_hscn.loader.synthetic import make_dataset
from graph_hscn.model.gps import GPS
from graph_hscn.model.mpnn import MPNN, build_mpnn
from graph_hscn.nn import functional as Fh
from graph_hscn.structure import build_category_index, category_index_of
from oracle import pyg_ops as P
from tests.helpers import DEV, F64_C, U32, KinkGuard, check_f64, grads_of, most_changed, referee_all, teeth

pytestmark = pytest.mark.gpu


def _lib_int(name):
    return int(getattr(_hip.lib(), name)())


def _offsets(cards):
    return [sum(cards[:c]) for c in range(len(cards) + 1)]


def _categories(cards, n, seed, ends=True):
    """[n, F] random categories; with ``ends`` every column hits its first (row 0) and last (row n - 1) category
    (a single row: the last)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([torch.randint(0, c, (n,), generator=g) for c in cards], 1) if n else torch.zeros(0, len(cards), dtype=torch.int64)
    if ends and n >= 1:
        x[n - 1] = torch.tensor(cards) - 1
    if ends and n >= 2:
        x[0] = 0
    return x


def _table(cards, D, seed):
    """Values distinct per row (row r sits near 3 r), so that an off-by-one in an offset cannot cancel."""
    R = sum(cards)
    return torch.randn(R, D, generator=torch.Generator().manual_seed(seed)) + 3.0 * torch.arange(R).unsqueeze(1)


# --------------------------------------------------------------------------- #
# 1. forward
# --------------------------------------------------------------------------- #
FORWARD_CASES = [(0, 9, 16), (1, 1, 4), (5, 3, 20), (67, 9, 64), (130, 9, 512)]
CARDS = {9: tuple(ATOM_FEATURE_DIMS), 3: tuple(BOND_FEATURE_DIMS), 1: (7,)}


@pytest.mark.parametrize("n,F,D", FORWARD_CASES)
def test_forward_equals_the_cpu_branch_bit_for_bit(n, F, D):
    cards = CARDS[F]
    W, idx = _table(cards, D, seed=n + D), _categories(cards, n, seed=n)
    ref = Fh.categorical_embed(W, idx, cards)
    got = Fh.categorical_embed(W.to(DEV), idx.to(DEV), cards)
    assert got.shape == (n, D) and torch.equal(got.cpu(), ref)
    Fh.check_categorical(DEV)


def test_forward_takes_a_non_contiguous_index_by_making_it_contiguous():
    cards = CARDS[3]
    W = _table(cards, 16, seed=1)
    wide = torch.zeros(40, 6, dtype=torch.int64)
    wide[:, ::2] = _categories(cards, 40, seed=2)
    view = wide.to(DEV)[:, ::2]
    assert not view.is_contiguous()
    enc = CategoricalEncoder(cards, 16).to(DEV)
    with torch.no_grad():
        enc.weight.copy_(W)
    ref = Fh.categorical_embed(W, wide[:, ::2].contiguous(), cards)
    assert torch.equal(enc(view).cpu(), ref)
    assert torch.equal(Fh.categorical_embed(W.to(DEV), view, cards).cpu(), ref)
    # and the backward finds the same items through the strided tensor
    Wd = W.to(DEV).requires_grad_(True)
    g = torch.randn(40, 16, generator=torch.Generator().manual_seed(3))
    Fh.categorical_embed(Wd, view, cards).backward(g.to(DEV))
    Wc = W.clone().requires_grad_(True)
    Fh.categorical_embed(Wc, wide[:, ::2].contiguous(), cards).backward(g)
    assert torch.equal(Wd.grad.cpu(), Wc.grad)           # rows of at most long_row() items: the CPU's own order


# --------------------------------------------------------------------------- #
# 2. index build
# --------------------------------------------------------------------------- #
def _check_index(idx, cards):
    n, F = idx.shape
    R = sum(cards)
    index = build_category_index(idx.to(DEV), cards)
    key = (idx + torch.tensor(_offsets(cards)[:-1])).flatten()
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=R)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    assert torch.equal(index.rowptr.cpu(), rowptr.to(torch.int32))
    assert torch.equal(index.item[: n * F].cpu(), (order // F).to(torch.int32))
    index.check()
    return index


def test_index_is_the_stable_sort_on_either_side_of_the_sort_chunk():
    S = _lib_int("hscn_catenc_sort_chunk")
    for n in (1, S - 1, S, S + 1, 4 * S + 3, 9 * S):          # (4 S + 3: a second workgroup; 9 S: whole chunks only)
        _check_index(_categories((13,), n, seed=n, ends=False), (13,))
    atoms = tuple(ATOM_FEATURE_DIMS)
    for n in (S // 9, S // 9 + 1, 700):                       # n F straddles a chunk; a node's columns across two chunks
        _check_index(_categories(atoms, n, seed=n), atoms)
    _check_index(torch.zeros(0, 3, dtype=torch.int64), CARDS[3])


def test_index_with_one_category_holding_everything_and_with_unused_categories():
    S = _lib_int("hscn_catenc_sort_chunk")
    bonds = CARDS[3]
    index = _check_index(torch.zeros(S + 77, 3, dtype=torch.int64), bonds)       # every item of a column in its row 0
    rp = index.rowptr.cpu()
    assert int(rp[1]) == S + 77 and int(rp[-1]) == 3 * (S + 77)
    x = _categories((5, 4096 - 5), 3000, seed=4, ends=False)                     # the widest table: 12 key bits
    x[:, 0] = torch.where(x[:, 0] == 2, torch.tensor(3), x[:, 0])                # category 2 of column 0 never used
    index = _check_index(x, (5, 4096 - 5))
    rp = index.rowptr.cpu()
    assert int(rp[3]) == int(rp[2])
    _check_index(torch.zeros(300, 1, dtype=torch.int64), (1,))                   # one table row: no key bits at all


# --------------------------------------------------------------------------- #
# 3. backward
# --------------------------------------------------------------------------- #
def _bwd_hip(idx, cards, g, D):
    W = torch.zeros(sum(cards), D, device=DEV, requires_grad=True)
    Fh.categorical_embed(W, idx, cards).backward(g)
    return W.grad.detach().cpu()


def _bwd_reference(idx, cards, g):
    """float64 on the same float32 cotangent: (dW64, mag = sum |g| per row, count per row, dW64 with every element's
    largest-magnitude term removed)."""
    n, F = idx.shape
    R, D = sum(cards), g.size(1)
    key = idx + torch.tensor(_offsets(cards)[:-1])
    g64 = g.double()
    ref = torch.zeros(R, D, dtype=torch.float64)
    mag = torch.zeros(R, D, dtype=torch.float64)
    big = torch.zeros(R, D, dtype=torch.float64)              # per element the term of largest magnitude
    for c in range(F):
        ref.index_add_(0, key[:, c], g64)
        mag.index_add_(0, key[:, c], g64.abs())
        for r in key[:, c].unique().tolist():
            rows = g64[key[:, c] == r]
            big[r] = rows.gather(0, rows.abs().argmax(0, keepdim=True)).squeeze(0)
    count = torch.bincount(key.flatten(), minlength=R)
    return ref, mag, count, ref - big


def _check_backward(idx, cards, g, what):
    ref, mag, count, dropped = _bwd_reference(idx, cards, g)
    n_terms = count.clamp(min=1).double().unsqueeze(1)
    assert int(count.max()) <= 2048
    # on the CPU reference, before comparing: the removed term of the longest row stands clear of that row's bound
    r = int(count.argmax())
    assert bool(((ref[r] - dropped[r]).abs() > 2.0 * F64_C * float(n_terms[r]) * U32 * mag[r]).all()), what
    got = _bwd_hip(idx.to(DEV), cards, g.to(DEV), g.size(1))
    check_f64(got, ref, mag, n_terms, dropped, what=what)
    assert bool((got[count == 0] == 0).all())                 # unused rows: exact zeros
    return got


def _row_length_case(extra, seed):
    """cards = (9,): category 0 holds ``extra`` items, categories 1..6 hold L-1, L, L+1, L+C-1, L+C, 3C+1 items,
    category 7 one item, category 8 none; shuffled.  Returns (idx [n, 1], the position of every item that is not in
    category 0, in order)."""
    L, C = _lib_int("hscn_catenc_long_row"), _lib_int("hscn_catenc_chunk")
    lengths = [extra, L - 1, L, L + 1, L + C - 1, L + C, 3 * C + 1, 1, 0]
    cats = torch.cat([torch.full((k,), c, dtype=torch.int64) for c, k in enumerate(lengths)])
    base = cats[cats != 0]
    base = base[torch.randperm(base.numel(), generator=torch.Generator().manual_seed(5))]      # the same for every `extra`
    if not extra:
        return base.unsqueeze(1), torch.arange(base.numel())
    slots = torch.randperm(base.numel() + extra, generator=torch.Generator().manual_seed(seed))
    where = slots[: base.numel()].sort().values               # the base items keep their order, the extras in between
    idx = torch.zeros(base.numel() + extra, dtype=torch.int64)
    idx[where] = base
    return idx.unsqueeze(1), where


@pytest.mark.parametrize("D", [4, 20, 64, 512])
def test_backward_at_the_long_row_and_chunk_edges(D):
    idx, _ = _row_length_case(0, 0)
    g = torch.randn(idx.size(0), D, generator=torch.Generator().manual_seed(D))
    _check_backward(idx, (9,), g, f"catenc bwd D={D}")


def test_backward_of_a_bond_shaped_batch_whose_items_all_share_one_row():
    n = 2048
    idx = torch.zeros(n, 3, dtype=torch.int64)
    g = torch.randn(n, 16, generator=torch.Generator().manual_seed(8))
    got = _check_backward(idx, CARDS[3], g, "catenc bwd, one row per column holds every item")
    offs = _offsets(CARDS[3])
    assert torch.equal(got[offs[0]], got[offs[1]]) and torch.equal(got[offs[0]], got[offs[2]])


def test_backward_of_an_atom_batch_and_an_empty_one():
    atoms = tuple(ATOM_FEATURE_DIMS)
    idx = _categories(atoms, 1500, seed=9)
    g = torch.randn(1500, 32, generator=torch.Generator().manual_seed(10))
    _check_backward(idx, atoms, g, "catenc bwd atoms n=1500")
    got = _bwd_hip(torch.zeros(0, 9, dtype=torch.int64, device=DEV), atoms, torch.zeros(0, 8, device=DEV), 8)
    assert got.shape == (sum(atoms), 8) and bool((got == 0).all())


def test_two_runs_and_two_batch_shapes_give_the_same_bits():
    D = 36
    idx_a, where_a = _row_length_case(0, 0)
    idx_b, where_b = _row_length_case(777, 11)               # the same items, 777 others in between and in front
    g_a = torch.randn(idx_a.size(0), D, generator=torch.Generator().manual_seed(12))
    g_b = torch.randn(idx_b.size(0), D, generator=torch.Generator().manual_seed(13))
    g_b[where_b] = g_a
    assert torch.equal(idx_b[where_b], idx_a)
    a1 = _bwd_hip(idx_a.to(DEV), (9,), g_a.to(DEV), D)
    a2 = _bwd_hip(idx_a.clone().to(DEV), (9,), g_a.to(DEV), D)
    assert torch.equal(a1, a2)
    b = _bwd_hip(idx_b.to(DEV), (9,), g_b.to(DEV), D)
    # every row but category 0's holds the same values in the same order, at other slots of the index
    assert torch.equal(a1[1:], b[1:])
    assert bool((a1[0] == 0).all()) and bool((b[0] != 0).any())


# --------------------------------------------------------------------------- #
# 4. the flag
# --------------------------------------------------------------------------- #
def test_an_index_outside_its_column_is_skipped_and_flagged():
    cards = CARDS[3]
    offs = _offsets(cards)
    n, D = 40, 16
    idx = _categories(cards, n, seed=14)
    idx[7, 1], idx[21, 1] = -1, cards[1]
    bad = torch.zeros(n, 3, dtype=torch.bool)
    bad[7, 1] = bad[21, 1] = True
    W = _table(cards, D, seed=15)
    Wc = W.clone().requires_grad_(True)
    ref = 0
    for c in range(3):                                       # the reference with the term zeroed
        term = Wc[offs[c]:offs[c + 1]].index_select(0, idx[:, c].clamp(0, cards[c] - 1))
        ref = ref + term * (~bad[:, c]).unsqueeze(1)
    Fh.check_categorical(DEV)
    Wd = W.to(DEV).requires_grad_(True)
    xd = idx.to(DEV)
    got = Fh.categorical_embed(Wd, xd, cards)
    assert torch.equal(got.detach().cpu(), ref.detach())
    with pytest.raises(IndexError):
        Fh.check_categorical(DEV)
    Fh.check_categorical(DEV)                                # read and cleared
    g = torch.randn(n, D, generator=torch.Generator().manual_seed(16))
    got.backward(g.to(DEV))
    ref.backward(g)
    assert torch.equal(Wd.grad.cpu(), Wc.grad)               # short rows: the CPU's own order, the two items left out
    index = category_index_of(xd, cards)
    assert int(index.rowptr[-1]) == 3 * n - 2
    with pytest.raises(IndexError):
        index.check()
    Fh.check_categorical(DEV)                                # the backward met no foreign slot


# --------------------------------------------------------------------------- #
# 5. models
# --------------------------------------------------------------------------- #
class _Toothed:
    """An encoder whose sum can leave one (row, column) term out: ``skip = (i, c)``."""
    skip = None

    def forward(self, x):
        out = super().forward(x)
        if self.skip is not None:
            i, c = self.skip
            keep = torch.zeros(x.size(0), 1, dtype=out.dtype)
            keep[i] = 1
            out = out - keep * self.weight[self.offsets[c] + int(x[i, c])]
        return out


class _Atom(_Toothed, AtomEncoder):
    pass


class _Bond(_Toothed, BondEncoder):
    pass


def _check_gates(g32, g64, what):
    """Every ReLU input of the float64 run farther from zero than 4 x the referee's own limit for its tensor."""
    assert set(g32) == set(g64) and g64
    for tag, v64 in g64.items():
        bound = 2.0 * float((g32[tag] - v64).abs().max()) + 8.0 * 2.0 ** -23 * float(v64.abs().max())
        kg = KinkGuard()
        kg.watch(tag, v64)
        kg.check(bound, what=f"{what} {tag}")


def _largest_term(enc, x):
    """The (i, c) whose table row has the largest norm among the rows the batch uses."""
    norms = torch.stack([enc.weight.detach()[enc.offsets[c] + x[:, c]].norm(dim=1) for c in range(x.size(1))], 1)
    k = int(norms.argmax())
    return k // x.size(1), k % x.size(1)


class AtomGCNRef(nn.Module):
    """MPNN(gcn, node_encoder="atom") restated: the encoder's CPU branch, oracle GCNConv layers H -> H -> ... -> C with
    a ReLU after every hidden one, then the per-graph mean / the node rows / the dot product of candidate pairs."""

    def __init__(self, H, C, L, task_level):
        super().__init__()
        self.node_encoder = _Atom(H)
        self.conv_layers = nn.ModuleList([P.GCNConv(H, H) for _ in range(L - 1)] + [P.GCNConv(H, C)])
        self.task_level = task_level
        self.watch = None

    def forward(self, x, edge_index, batch, num_graphs, pairs=None):
        h = self.node_encoder(x)
        for i, conv in enumerate(self.conv_layers[:-1]):
            h = conv(h, edge_index)
            if self.watch is not None:
                self.watch(f"layer {i} relu input", h)
            h = torch.relu(h)
        h = self.conv_layers[-1](h, edge_index)
        if self.task_level == "node":
            return h
        if self.task_level == "link":
            return (h[pairs[0]] * h[pairs[1]]).sum(1)
        return P.global_mean_pool(h, batch, num_graphs)


# chosen on the CPU, from the reference alone: of the seeds 0..5 the one whose float64 run keeps its ReLU inputs farthest
# from zero (8 x the required distance; seed 0 does not meet the condition)
MPNN_SEEDS = {"graph": 1, "node": 1, "link": 1}
MPNN_H, MPNN_L = 16, 3
MPNN_WIDTH = {"graph": 10, "node": 10, "link": 8}     # (the pair decoder takes a multiple of 4)


def _peptides(seed):
    graphs = make_dataset("peptides_func", 4, seed=seed, edge_features=True)
    b = Batch.from_data_list(graphs)
    assert b.x.dtype == torch.int64 and b.edge_attr.dtype == torch.int64
    return graphs, b


def _pairs(b, seed):
    """Candidate pairs inside every graph of the batch (peptides graphs carry none of their own): [2, 64]."""
    g = torch.Generator().manual_seed(seed)
    ptr = b.ptr.tolist()
    out = []
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        out.append(torch.randint(lo, hi, (2, 16), generator=g))
    return torch.cat(out, 1)


def _mpnn_reference(level):
    """Everything of a model case that is computed on the CPU (the seed search runs this alone)."""
    seed = MPNN_SEEDS[level]
    _, b = _peptides(seed)
    torch.manual_seed(seed)
    C = MPNN_WIDTH[level]
    ref = AtomGCNRef(MPNN_H, C, MPNN_L, level)
    pairs = _pairs(b, seed) if level == "link" else None
    rows = {"graph": (int(b.num_graphs), C), "node": (int(b.num_nodes), C)}.get(level) or (int(pairs.size(1)),)
    gy = torch.randn(*rows, generator=torch.Generator().manual_seed(1))

    def run(dtype, skip=None):
        m = copy.deepcopy(ref).to(dtype)
        m.node_encoder.skip = skip
        seen = {}
        m.watch = lambda tag, t: seen.__setitem__(tag, t.detach().double())
        out = m(b.x, b.edge_index, b.batch, int(b.num_graphs), pairs)
        out.backward(gy.to(dtype))
        return {"p." + n: p.grad.detach().clone() for n, p in m.named_parameters()}, out.detach(), seen

    skip = _largest_term(ref.node_encoder, b.x)
    return ref, b, pairs, gy, run(torch.float32), run(torch.float64), run(torch.float64, skip)


@pytest.mark.parametrize("level", ["graph", "node", "link"])
def test_mpnn_with_the_atom_encoder_under_the_float64_referee(level):
    from graph_hscn.train import batching
    what = f"MPNN gcn + AtomEncoder, {level} level"
    ref, b, pairs, gy, (o32, y32, g32), (o64, y64, g64), (d64, dy64, _) = _mpnn_reference(level)
    assert len(g64) == MPNN_L - 1
    _check_gates(g32, g64, what)
    pm = MPNN(CONV_DICT["gcn"], ACT_DICT["relu"], 9, MPNN_H, MPNN_WIDTH[level], MPNN_L, dropout=0.0, task_level=level,
              node_encoder="atom").to(DEV)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    if pairs is not None:
        b.edge_label_index = pairs
    bd = batching.to_device(pm, b, DEV)
    assert bd.x.dtype == torch.int64
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": dy64}, what)
    got = grads_of(pm)
    assert all(v is not None for v in got.values()) and len(got) == 1 + 2 * MPNN_L
    referee_all(got, o32, o64, what)
    reached = most_changed(o64, [d64])
    # the removed term reaches every tensor but the last bias: behind the mean pool (and at node level, as the plain sum
    # of the cotangent rows) its gradient does not depend on the forward values
    assert set(o64) - set(reached) <= {f"p.conv_layers.{MPNN_L - 1}.bias"}, sorted(set(o64) - set(reached))
    teeth(got, o32, o64, reached, what)
    # categories absent from the batch: exact zeros
    used = torch.bincount((b.x + torch.tensor(_offsets(ATOM_FEATURE_DIMS)[:-1])).flatten(), minlength=sum(ATOM_FEATURE_DIMS))
    assert bool((used == 0).any())
    assert bool((got["p.node_encoder.weight"][used == 0] == 0).all())
    pm.check_flags()


# ---- GPS with the gated local branch, AtomEncoder and BondEncoder ------------------------------------------------------
GPS_D, GPS_HEADS, GPS_L = 16, 4, 2
# Chosen on the CPU, from the reference alone: of the seeds 0..23 the float64 run keeps its gates the required distance
# away for 2, 5, 16 and 22 (1.2, 2.0, 1.4, 1.1 x); 5 has the widest margin, and its batch-norm inputs
# (tests/test_gpu_gatedgcn.py's second condition) stay within |mean| <= 1.6 std.
GPS_SEED = 5


def _gps_reference():
    from tests import gatedgcn_oracle as GG
    from tests.test_gpu_attention import _Terms
    from tests.test_gpu_gatedgcn import _watch_cotangent
    _, b = _peptides(GPS_SEED)
    torch.manual_seed(GPS_SEED)
    ref = GG.GatedGPSRef(9, GPS_D, 10, GPS_L, GPS_HEADS, edge_dim=3)
    ref.node_encoder, ref.edge_encoder = _Atom(GPS_D), _Bond(GPS_D)
    gy = torch.randn(int(b.num_graphs), 10, generator=torch.Generator().manual_seed(1))
    bias_keys = {f"p.layers.{i}.conv.{n}.bias": (i, n) for i in range(GPS_L) for n in "AB"}

    def run(dtype, terms=False, atom_skip=None, bond_skip=None, **skips):
        m = copy.deepcopy(ref).to(dtype)
        m.train()                                          # the gated layers' batch norms in training mode
        m.node_encoder.skip, m.edge_encoder.skip = atom_skip, bond_skip
        seen, cot = {}, {"bn mean / std": 0.0}
        m.set_watch(lambda tag, t: seen.__setitem__(tag, t.detach().double()))
        hooks = [_watch_cotangent(getattr(m.layers[i].conv, n), cot, k) for k, (i, n) in bias_keys.items()]
        for layer in m.layers:
            for bn in (layer.conv.bn_node_x, layer.conv.bn_edge_e):
                hooks.append(bn.register_forward_hook(lambda mod, a, out: cot.__setitem__(
                    "bn mean / std", max(cot["bn mean / std"],
                                         float((a[0].detach().mean(0).abs() / a[0].detach().std(0)).max())))))
        tm = None
        if terms:
            tm = _Terms(m)
            # as tests/test_gpu_gatedgcn.py counts them: per gated layer the two sums over the largest in-degree, the
            # sigmoid, the quotient and the final addition (+ 8); the pool's segment; and the encoders' F adds
            tm.chain += GPS_L * (int(torch.bincount(b.edge_index[1]).max()) + 8) + int(torch.bincount(b.batch).max()) + 9 + 3
        out = m(b.x, b.edge_index, b.edge_attr, b.batch, b.ptr, int(b.num_graphs), None, **skips)
        out.backward(gy.to(dtype))
        for h in hooks:
            h.remove()
        if tm is not None:
            tm.close()
        g = {"p." + n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}
        return g, out.detach(), seen, cot, tm

    return ref, b, gy, bias_keys, run


def test_gps_with_atom_and_bond_encoders_under_the_float64_referee():
    from graph_hscn.train import batching
    from tests.test_gpu_gatedgcn import _A_BIAS, _B_BIAS, _NORM_WEIGHT, BN_MEAN_OVER_STD, _row_dropped
    what = "GPS local_conv=gatedgcn + AtomEncoder + BondEncoder, graph level"
    ref, b, gy, bias_keys, run = _gps_reference()
    o32, y32, g32, _, _ = run(torch.float32)
    o64, y64, g64, cot, terms = run(torch.float64, terms=True)
    assert len(g64) == GPS_L * 3 + 1
    _check_gates(g32, g64, what)
    print(f"   {what}: largest |mean| / std of a batch-norm input column = {cot['bn mean / std']:.2f}")
    assert cot["bn mean / std"] <= BN_MEAN_OVER_STD
    atom_drop = run(torch.float64, atom_skip=_largest_term(ref.node_encoder, b.x))
    bond_drop = run(torch.float64, bond_skip=_largest_term(ref.edge_encoder, b.edge_attr))
    edge_drop = run(torch.float64, skip=int(b.edge_index.size(1)) // 2)
    drops = [atom_drop[0], bond_drop[0], edge_drop[0], run(torch.float64, att_skip=(0, 0))[0],
             run(torch.float64, pool_skip=0)[0]]
    drops += [_row_dropped(o64, k, cot[k]) for k in bias_keys]
    pm = GPS(9, GPS_D, 10, GPS_L, num_heads=GPS_HEADS, local_conv="gatedgcn", activation=ACT_DICT["relu"], dropout=0.0,
             norm="layer", node_encoder="atom", edge_encoder="bond").to(DEV).train()
    bd = batching.to_device(pm, b, DEV)
    assert bd.x.dtype == torch.int64 and bd.edge_attr.dtype == torch.int64
    for layer in pm.layers:
        layer.conv.C.materialize(GPS_D, bd.x)
    pm.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    pred = pm(bd)
    assert pm.last_engine == "layered" and pred.shape == y64.shape
    pred.backward(gy.to(DEV))
    referee_all({"pred": pred}, {"pred": y32}, {"pred": y64}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": atom_drop[1]}, what)
    teeth({"pred": pred}, {"pred": y32}, {"pred": y64}, {"pred": bond_drop[1]}, what)
    got = grads_of(pm)
    none = {f"p.layers.{GPS_L - 1}.conv.bn_edge_e.{n}" for n in ("weight", "bias")}
    assert {k for k, v in o64.items() if v is None} == none
    # the cancelling sums of tests/test_gpu_gatedgcn.py's GPS case, named with their reasons there
    cancelling = {f"p.layers.{i}.attn.in_proj_bias": "the K third is zero in exact arithmetic (tests/test_gpu_attention.py)"
                  for i in range(GPS_L)}
    cancelling[f"p.layers.{GPS_L - 1}.norm2.bias"] = "equal parts of differing sign behind the mean pool (test_gpu_attention.py)"
    cancelling.update({k: (_A_BIAS if n == "A" else _B_BIAS) for k, (_, n) in bias_keys.items()})
    cancelling.update({f"p.layers.{i}.conv.{n}.weight": _NORM_WEIGHT for i in range(GPS_L) for n in "AB"})
    referee_all(got, o32, o64, what, terms=terms, cancelling=list(cancelling))
    terms.bound_teeth(got, o32, o64, drops, list(cancelling), what)
    for name, drop in (("atom", atom_drop), ("bond", bond_drop)):
        reached = most_changed(o64, [drop[0]])
        assert {"p.node_encoder.weight", "p.edge_encoder.weight", "p.layers.0.conv.C.weight", "p.lin_2.weight"} <= set(reached), \
            (name, sorted(reached))
        teeth(got, o32, o64, {k: v for k, v in reached.items() if k not in cancelling}, f"{what} [{name} term]")
    for key, x, dims in (("p.node_encoder.weight", b.x, ATOM_FEATURE_DIMS), ("p.edge_encoder.weight", b.edge_attr, BOND_FEATURE_DIMS)):
        used = torch.bincount((x + torch.tensor(_offsets(dims)[:-1])).flatten(), minlength=sum(dims))
        assert bool((got[key][used == 0] == 0).all())
    pm.check_flags()


# --------------------------------------------------------------------------- #
# 6. the training loop and the resident entry points
# --------------------------------------------------------------------------- #
def test_two_epochs_through_the_training_loop_and_the_resident_entry_points_refuse():
    from types import SimpleNamespace

    from graph_hscn.step import MPNNResidentTrainStep
    from graph_hscn.train import batching
    from graph_hscn.train.eval_resident import DeviceEvaluator
    from graph_hscn.train.train import train
    from graph_hscn.train.train_resident import fit_resident
    graphs = make_dataset("peptides_func", 8, seed=3)
    torch.manual_seed(3)
    pm = build_mpnn(MPNNConfig("gcn", "relu", dropout=0.1, node_encoder="atom"), 9, 10).to(DEV)
    before = pm.node_encoder.weight.detach().clone()
    cfg = SimpleNamespace(model_type="mpnn", epochs=2, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0,
                          metric="ap")
    opt = SimpleNamespace(optim_type="adam", lr=1e-3, weight_decay=0.0, batch_accumulation=1, clip_grad_norm=False,
                          scheduler=None)
    loaders = [DataLoader(graphs, 4), DataLoader(graphs, 8)]
    history = train(None, opt, cfg, loaders, pm)
    assert len(history) == 2 and all(np.isfinite(h[0]) for h in history)
    assert not torch.equal(pm.node_encoder.weight.detach(), before)
    pm.check_flags()
    # the resident entry points refuse the model, and say why
    bd = batching.to_device(pm, Batch.from_data_list(graphs[:4]), DEV)
    pm.engine = "auto"
    with torch.no_grad():
        out = pm(bd)
    assert pm.last_engine == "layered" and out.shape == (4, 10)
    pm.engine = "resident"
    with torch.no_grad(), pytest.raises(RuntimeError, match="categorical input encoder"):
        pm(bd)
    pm.engine = "layered"
    with pytest.raises(RuntimeError, match="categorical input encoder"):
        MPNNResidentTrainStep(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="categorical input encoder"):
        batching.resident_step(pm, bd, "cross_entropy")
    with pytest.raises(RuntimeError, match="categorical input encoder"):
        DeviceEvaluator(graphs, pm, "cross_entropy", 4).run()
    cfg1 = SimpleNamespace(epochs=1, eval_period=1, loss_fn="cross_entropy", patience=10, min_delta=0.0)
    with pytest.raises(RuntimeError, match="categorical input encoder"):
        fit_resident(None, opt, cfg1, graphs, [], pm, 4)
