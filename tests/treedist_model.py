"""An independent model of the tree distance accumulator, written from the definitions alone.

The splits of a tree are Python `frozenset`s of taxa from a traversal of its own (`splits`): no bit masks, no popcount,
no library call.  shared = len(A & B), rf = len(A ^ B) on sets of frozensets; a column is a distinct split found in at
least two trees.

    splits(parent, T)              # set of frozensets: the side without taxon 0, 2 <= size <= T - 2
    expected(trees, T)             # (nsplits i64[N], shared i64[N, N], rf i64[N, N], columns)
    set_model(T, seed)             # (trees, nsplits, shared, rf, columns) of consensus_model.tree_set, computed once
    assert_matches(acc, model)     # the accumulator's three arrays against the model's
    nni_pairs(T, n, seed)          # n independent random binary trees, each followed by one NNI of itself
    newick_of(parent, T)           # numeric newick text of a parent array

Generators come from consensus_model / concordance_split_model.
"""
from __future__ import annotations

from collections import Counter
from functools import lru_cache

import numpy as np

import consensus_model as cm


def splits(parent, T):
    """For every node the taxa below it, found by walking up from every tip; named by the side without taxon 0."""
    parent = [int(p) for p in parent]
    below = [set() for _ in parent]
    for t in range(T):
        v = t
        while v >= 0:
            below[v].add(t)
            v = parent[v]
    everyone = frozenset(range(T))
    out = set()
    for s in below:
        side = frozenset(s)
        if 0 in side:
            side = everyone - side
        if 2 <= len(side) <= T - 2:
            out.add(side)
    return out


def expected(trees, T):
    sets = [splits(p, T) for p in trees]
    N = len(sets)
    nsplits = np.array([len(s) for s in sets], np.int64)
    shared = np.zeros((N, N), np.int64)
    rf = np.zeros((N, N), np.int64)
    for i in range(N):
        for j in range(N):
            shared[i, j] = len(sets[i] & sets[j])
            rf[i, j] = len(sets[i] ^ sets[j])
    seen = Counter()
    for s in sets:
        seen.update(s)
    columns = sum(1 for c in seen.values() if c >= 2)
    return nsplits, shared, rf, columns


@lru_cache(maxsize=None)
def set_model(T, seed):
    trees = cm.tree_set(T, seed)
    out = (trees,) + expected(trees, T)
    for a in out[1:4]:
        a.setflags(write=False)
    return out


def assert_matches(acc, nsplits, shared, rf):
    np.testing.assert_array_equal(acc.nsplits(), nsplits)
    np.testing.assert_array_equal(acc.shared(), shared)
    np.testing.assert_array_equal(acc.rf(), rf)
    assert acc.ntrees == len(nsplits)


def nni_pairs(T, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t = cm.random_binary(T, rng)
        out.append(t)
        out.append(cm.nni(t, T, rng))
    return out


def newick_of(parent, T):
    kids = cm.kids_of(parent)
    root = [int(p) for p in parent].index(-1)

    def text(v):
        return str(v) if v < T else "(" + ",".join(text(k) for k in kids[v]) + ")"

    return text(root) + ";"
