"""Seeded synthetic LRGB-shaped graphs.

The reference's datasets (graph_hscn/loader/dataset/peptides_functional.py:21-115,
peptides_structural.py:21-121) need network + rdkit + ogb; none exist on the
build or GPU boxes.  These generators reproduce only the *shape* statistics of
the LRGB sets: node-count distribution, directed edge
count, feature width/type, label width.  Edge lists follow the OGB
``smiles2graph`` layout: undirected bonds emitted as adjacent (i,j),(j,i) pairs,
no self loops, no duplicates.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ..data import Data

# OGB atom feature cardinalities (9 integer columns)
_ATOM_CARD = np.array([119, 5, 12, 12, 10, 6, 6, 2, 2])
# OGB bond feature cardinalities (3 integer columns: bond type, stereo, conjugation)
_BOND_CARD = np.array([5, 6, 2])
# edge feature width of the "normal" (superpixel) shapes: float boundary statistics
_NORMAL_EDGE_DIM = 2


@dataclass(frozen=True)
class Shape:
    name: str
    n_mean: float
    n_std: float
    n_min: int
    n_max: int
    und_per_node: float      # undirected edges per node (directed = 2x)
    num_features: int
    feature_kind: str        # "atom" (int columns) | "normal" (float)
    num_classes: int
    task: str                # "multilabel" | "regression" | "node_class" (one class index per NODE) | "link"


SHAPES = {
    # n ~ 150.94, e ~ 307.30 directed
    "peptides_func": Shape("peptides_func", 151.0, 84.0, 8, 444, 1.018, 9, "atom", 10, "multilabel"),
    "peptides_struct": Shape("peptides_struct", 151.0, 84.0, 8, 444, 1.018, 9, "atom", 11, "regression"),
    # n ~ 479.40, e ~ 2710.48 directed
    "pascalvoc_sp": Shape("pascalvoc_sp", 479.0, 60.0, 395, 500, 2.827, 14, "normal", 21, "multilabel"),
    # n ~ 30.14, e ~ 61.09 directed
    "pcqm_contact": Shape("pcqm_contact", 30.0, 8.0, 9, 53, 1.013, 9, "atom", 1, "regression"),
}

# Node-level shapes (``y`` is one class index per node, int64 [n]), kept apart from the graph-level table:
# PascalVOC-SP with the dataset's real task -- one of 21 classes per superpixel, weighted cross-entropy scored by
# macro-F1 in the LRGB recipe.  The graphs are "pascalvoc_sp"'s.
NODE_SHAPES = {
    "pascalvoc_sp_node": Shape("pascalvoc_sp_node", 479.0, 60.0, 395, 500, 2.827, 14, "normal", 21, "node_class"),
}

# Link-level shapes (``edge_label_index`` int64 [2, P] candidate pairs with ``edge_label`` float32 [P]; no ``y``), kept
# apart as well: PCQM-Contact with the dataset's real task -- which pairs of atoms are in contact -- scored by a
# per-graph MRR.  The graphs are "pcqm_contact"'s, node for node and edge for edge.
LINK_SHAPES = {
    "pcqm_contact_link": Shape("pcqm_contact_link", 30.0, 8.0, 9, 53, 1.013, 9, "atom", 1, "link"),
}
# an unordered candidate pair {u, v} is a contact with this probability, whatever the graph: about 3 % of the
# candidates are positive, and a molecule of ten atoms (some 35 candidate pairs) has none one time in three
LINK_POSITIVE_PROB = 0.03


def _molecule_edges(rng: np.random.Generator, n: int, n_und: int) -> np.ndarray:
    """Random tree with SMILES-like locality plus ring closures -> [2, 2*m]."""
    und = set()
    for i in range(1, n):
        if rng.random() < 0.8:
            p = i - 1
        else:
            p = int(rng.integers(max(0, i - 12), i))
        und.add((p, i))
    tries = 0
    while len(und) < n_und and tries < 20 * n_und and n > 3:
        tries += 1
        i = int(rng.integers(0, n - 2))
        j = i + int(rng.integers(2, min(8, n - i)))
        if j < n:
            und.add((i, j))
    und = sorted(und, key=lambda e: (e[1], e[0]))
    ei = np.empty((2, 2 * len(und)), dtype=np.int64)
    for k, (i, j) in enumerate(und):
        ei[:, 2 * k] = (i, j)
        ei[:, 2 * k + 1] = (j, i)
    return ei


def _lattice_edges(rng: np.random.Generator, n: int, n_und: int) -> np.ndarray:
    """Superpixel-adjacency-like graph: nodes on a ~sqrt(n) wide strip, edges to
    near neighbours in index space."""
    w = max(2, int(round(np.sqrt(n))))
    und = set()
    for i in range(n):
        if i + 1 < n and (i + 1) % w:
            und.add((i, i + 1))
        if i + w < n:
            und.add((i, i + w))
    tries = 0
    while len(und) < n_und and tries < 20 * n_und:
        tries += 1
        i = int(rng.integers(0, n - 1))
        j = i + int(rng.choice([w - 1, w + 1, 2, 2 * w]))
        if j < n:
            und.add((i, j))
    und = sorted(und)
    ei = np.empty((2, 2 * len(und)), dtype=np.int64)
    for k, (i, j) in enumerate(und):
        ei[:, 2 * k] = (i, j)
        ei[:, 2 * k + 1] = (j, i)
    return ei


def _node_class_probs(num_classes: int) -> np.ndarray:
    """A fixed skewed class distribution, p_c proportional to 0.6^c (PascalVOC-SP is dominated by its background
    class): class weights matter, and the rare classes are missing from a small batch."""
    p = 0.6 ** np.arange(num_classes, dtype=np.float64)
    return p / p.sum()


def _hop_distances(n: int, ei: np.ndarray) -> np.ndarray:
    """[n, n] hop distances by a BFS from every node (n for unreachable)."""
    adj = [[] for _ in range(n)]
    for a, b in zip(ei[0].tolist(), ei[1].tolist()):
        adj[a].append(b)
    dist = np.full((n, n), n, dtype=np.int64)
    for s in range(n):
        dist[s, s] = 0
        frontier = [s]
        while frontier:
            nxt = []
            for a in frontier:
                for b in adj[a]:
                    if dist[s, b] == n:
                        dist[s, b] = dist[s, a] + 1
                        nxt.append(b)
            frontier = nxt
    return dist


def _link_labels(rng: np.random.Generator, n: int, ei: np.ndarray, prob: float = None):
    """Candidates: every ordered pair (u, v), u != v, at hop distance >= 2, in (u, v) order.  Labels are symmetric:
    one draw per unordered pair serves (u, v) and (v, u)."""
    dist = _hop_distances(n, ei)
    u, v = np.nonzero(dist >= 2)                        # row-major: ascending (u, v); the diagonal has distance 0
    draw = rng.random((n, n)) < (LINK_POSITIVE_PROB if prob is None else prob)
    contact = np.triu(draw, 1)
    contact = contact | contact.T
    index = np.stack([u, v]).astype(np.int64)
    return torch.from_numpy(index), torch.from_numpy(contact[u, v].astype(np.float32))


def _edge_features(rng: np.random.Generator, shape: Shape, ei: np.ndarray) -> torch.Tensor:
    """One feature row per undirected bond, carried by both of its directions (the adjacent columns (i, j), (j, i) of
    ``ei``): int64 [E, 3] bond columns for "atom" shapes, float32 [E, 2] for "normal" ones."""
    m = ei.shape[1] // 2
    if shape.feature_kind == "atom":
        und = np.stack([rng.integers(0, c, size=m) for c in _BOND_CARD], 1).astype(np.int64)
    else:
        und = rng.normal(size=(m, _NORMAL_EDGE_DIM)).astype(np.float32)
    return torch.from_numpy(np.repeat(und, 2, axis=0))


def make_graph(rng: np.random.Generator, shape: Shape, n: Optional[int] = None,
               label_rng: Optional[np.random.Generator] = None, edge_features: bool = False,
               edge_rng: Optional[np.random.Generator] = None) -> Data:
    """``label_rng`` (link shapes): the generator of the label draws; ``make_dataset`` passes a stream of its own, so
    that the graph stream ``rng`` is spent exactly as the graph-level shape spends it.  ``edge_features``: the graph
    also gets ``edge_attr`` (``_edge_features``), drawn from ``edge_rng`` -- a stream of its own again, so that the
    graph is the same with and without them; without one, a generator seeded from the graph's edge count serves."""
    g = _make_graph(rng, shape, n, label_rng)
    if edge_features:
        ei = g.edge_index.numpy()
        g.edge_attr = _edge_features(edge_rng if edge_rng is not None else np.random.default_rng([ei.shape[1], 2]),
                                     shape, ei)
    return g


def _make_graph(rng: np.random.Generator, shape: Shape, n: Optional[int],
                label_rng: Optional[np.random.Generator]) -> Data:
    if n is None:
        n = int(np.clip(round(rng.normal(shape.n_mean, shape.n_std)), shape.n_min, shape.n_max))
    n_und = max(n - 1, int(round(shape.und_per_node * n)))
    if shape.feature_kind == "atom":
        ei = _molecule_edges(rng, n, n_und)
        x = torch.from_numpy(
            np.stack([rng.integers(0, c, size=n) for c in _ATOM_CARD[: shape.num_features]], 1).astype(np.int64))
    else:
        ei = _lattice_edges(rng, n, n_und)
        x = torch.from_numpy(rng.normal(size=(n, shape.num_features)).astype(np.float32))
    if shape.task == "link":
        rng.normal(size=(1, shape.num_classes))         # the draw "pcqm_contact" spends on its target: same graphs after
        index, label = _link_labels(label_rng if label_rng is not None else rng, n, ei)
        return Data(x=x, edge_index=torch.from_numpy(ei), num_nodes=n, edge_label_index=index, edge_label=label)
    if shape.task == "node_class":
        y = torch.from_numpy(rng.choice(shape.num_classes, size=n, p=_node_class_probs(shape.num_classes)).astype(np.int64))
    elif shape.task == "multilabel":
        y = torch.from_numpy((rng.random((1, shape.num_classes)) < 0.2).astype(np.float32))
    else:
        y = torch.from_numpy(rng.normal(size=(1, shape.num_classes)).astype(np.float32))
    return Data(x=x, edge_index=torch.from_numpy(ei), y=y, num_nodes=n)


def make_dataset(name: str, num_graphs: int, seed: int = 0, edge_features: bool = False) -> List[Data]:
    """``num_graphs`` seeded graphs of the named LRGB shape.  ``edge_features``: every graph also carries
    ``edge_attr``, drawn from a generator of its own (``[seed, 2]``): ``x``, ``edge_index`` and the targets are the
    same bits with and without it."""
    shape = SHAPES[name] if name in SHAPES else (NODE_SHAPES[name] if name in NODE_SHAPES else LINK_SHAPES[name])
    rng = np.random.default_rng(seed)
    label_rng = np.random.default_rng([seed, 1]) if shape.task == "link" else None
    edge_rng = np.random.default_rng([seed, 2]) if edge_features else None
    return [make_graph(rng, shape, label_rng=label_rng, edge_features=edge_features, edge_rng=edge_rng)
            for _ in range(num_graphs)]
