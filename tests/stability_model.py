"""An independent model of the leaf stability accumulator, written from the definitions alone on
top of `qdist_model.codes` (a tree as its splits as taxon sets): no depths, no bit planes, no popcounts, no library call.

    code_array(trees, T, quartets)   # i8 [N, Q]: the code of every quartet row in every tree
    counts_of(code)                  # i64 [Q, 4]: per row the trees with code 0, 1, 2, 3, by comparing codes
    measures(counts)                 # (res, top, dif) i64 [Q] each; top and second by sorting
    acc_of(counts, quartets, T)      # i64 [T, 4] = (quartets, res, top, dif) per taxon, by numpy.add.at
    expected(trees, T, quartets)     # (counts, acc)
    set_model(T, seed)               # (trees, quartets, ranks or None, counts, acc) of consensus_model.tree_set, once
    stability(acc, N, kind)          # f64 [T]
    permuted_counts(counts, perm)    # the counts of rows whose taxa were given as row[perm]
    dominant_splits(quartets, counts, min_count)   # plain Python
    assert_matches(acc_object, counts_table, want_counts, want_acc, N)
    rogue_set(T)                     # a caterpillar on 0..T-2 with taxon T-1 grafted onto each of its 2T-5 edges
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import consensus_model as cm
import qdist_model as qm

KIND_COLUMN = {"res": 1, "max": 2, "dif": 3}


def code_array(trees, T, quartets):
    if not len(trees):
        return np.zeros((0, len(quartets)), np.int8)
    return np.stack([qm.codes(p, T, quartets) for p in trees])


def counts_of(code):
    return np.stack([(code == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int64)


def measures(counts):
    counts = np.asarray(counts, np.int64)
    ordered = np.sort(counts[:, :3], axis=1)
    top, second = ordered[:, 2], ordered[:, 1]
    return counts[:, :3].sum(axis=1), top, top - second


def acc_of(counts, quartets, T):
    res, top, dif = measures(counts)
    acc = np.zeros((T, 4), np.int64)
    q = np.asarray(quartets, np.int64)
    for k in range(4):
        np.add.at(acc[:, 0], q[:, k], 1)
        np.add.at(acc[:, 1], q[:, k], res)
        np.add.at(acc[:, 2], q[:, k], top)
        np.add.at(acc[:, 3], q[:, k], dif)
    return acc


def expected(trees, T, quartets):
    counts = counts_of(code_array(trees, T, quartets))
    return counts, acc_of(counts, quartets, T)


@lru_cache(maxsize=None)
def set_model(T, seed):
    trees, quartets, ranks = qm.set_model(T, seed)[:3]
    out = (trees, quartets, ranks) + expected(trees, T, quartets)
    for a in out[3:]:
        a.setflags(write=False)
    return out


def stability(acc, N, kind):
    out = np.zeros(len(acc), np.float64)
    for t, row in enumerate(acc):
        if row[0] and N:
            out[t] = int(row[KIND_COLUMN[kind]]) / (N * int(row[0]))
    return out


# the code of the pairing {x, y} | rest, by the positions x < y of the pair that holds position 0's partner
_CODE_OF_PARTNER = {1: 0, 2: 1, 3: 2}


def permuted_counts(counts, perm):
    """The rows were given as row[perm] (new position i holds the taxon of old position perm[i]).  The new code k pairs
    new positions 0 and k + 1, that is old positions perm[0] and perm[k + 1]; the old code of that pairing is named by the
    partner of old position 0."""
    counts = np.asarray(counts)
    out = counts.copy()
    for k in range(3):
        pair = {perm[0], perm[k + 1]}
        if 0 not in pair:
            pair = set(range(4)) - pair
        (partner,) = pair - {0}
        out[:, k] = counts[:, _CODE_OF_PARTNER[partner]]
    return out


def dominant_splits(quartets, counts, min_count=1):
    splits, weights = [], []
    for (a, b, c, d), row in zip(np.asarray(quartets).tolist(), np.asarray(counts).tolist()):
        n = row[:3]
        top = max(n)
        if n.count(top) != 1 or top < min_count:
            continue
        splits.append([(a, b, c, d), (a, c, b, d), (a, d, b, c)][n.index(top)])
        weights.append(float(top))
    return np.array(splits, np.uint32).reshape(-1, 4), np.array(weights, np.float64)


def assert_matches(acc, table, want_counts, want_acc, N):
    """The accumulator's sums (and, where one was returned, a counts table) against the model's, exactly."""
    raw = acc.raw()
    assert raw.dtype == np.uint64 and raw.shape == (acc.ntaxa, 4)
    np.testing.assert_array_equal(raw.astype(np.int64), want_acc)
    np.testing.assert_array_equal(acc.quartets_per_taxon(), want_acc[:, 0])
    if table is not None:
        assert table.dtype == np.uint16 and table.shape == want_counts.shape
        np.testing.assert_array_equal(table.astype(np.int64), want_counts)
    assert acc.ntrees == N
    for kind in KIND_COLUMN:
        np.testing.assert_array_equal(acc.stability(kind), stability(want_acc, N, kind))


def graft(parent, T, edge_child, tip):
    """The tree on taxa 0..T-2 (`parent`, T - 1 taxa) with taxon `tip` = T - 1 put on the edge above `edge_child`.  Taxa
    keep their numbers, internal nodes move up by one, and the new internal node comes last."""
    old = [int(p) for p in parent]
    shift = lambda v: v if v < T - 1 else v + 1      # noqa: E731
    new = [0] * (len(old) + 2)
    for v, p in enumerate(old):
        new[shift(v)] = -1 if p < 0 else shift(p)
    mid = len(old) + 1
    new[mid] = new[shift(edge_child)]
    new[shift(edge_child)] = mid
    new[tip] = mid
    return np.array(new, np.int32)


@lru_cache(maxsize=None)
def rogue_set(T):
    """The unrooted caterpillar on 0..T-2 has 2 (T - 1) - 3 = 2T - 5 edges; one tree per edge, taxon T - 1 on it."""
    base = cm.unrooted(cm.caterpillar(T - 1), T - 1)
    edges = [v for v, p in enumerate(base) if p >= 0]
    assert len(edges) == 2 * T - 5
    return [graft(base, T, v, T - 1) for v in edges]
