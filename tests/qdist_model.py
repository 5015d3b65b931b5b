"""An independent model of the quartet distance accumulator, written from the definitions alone:
no depths, no lowest common ancestors, no bit planes, no popcount, no library call.

A tree is its set of splits as taxon sets, from a walk up from every tip (as treedist_model).  A tree displays the pairing
a,b|c,d of four taxa iff one of its splits has a and b on one side and c and d on the other; the code of (a, b, c, d) is
0 for a,b|c,d, 1 for a,c|b,d, 2 for a,d|b,c and 3 when no split separates any pairing.  Per split one numpy boolean
indicator vector over the taxa does this for all quartets at once.  The five classes A..E come from comparing the code
arrays of two trees.

    unrank(ranks, T)                 # i32 [Q, 4]: lexicographic rank -> 4-combination
    all_quartets(T)                  # i32 [C(T,4), 4] in rank order
    codes(parent, T, quartets)       # i8 [Q]
    expected(trees, T, quartets)     # (A, B, C, D, E) i64 [N, N] each
    set_model(T, seed)               # (trees, quartets, ranks or None, A, B, C, D, E) of consensus_model.tree_set, once
    assert_matches(acc, classes, Q)  # the accumulator's arrays against the model's
    nni_parts(t1, t2, T)             # the sizes of the four subtrees around the edge two trees one NNI apart differ in
    contract(parent, T, side)        # the tree with the edge of split `side` contracted
"""
from __future__ import annotations

from functools import lru_cache
from itertools import combinations
from math import comb

import numpy as np

import consensus_model as cm
import treedist_model as dm

FULL_T = 33             # up to here the sets score all quartets, above SAMPLE sampled ranks
SAMPLE = 3000


def unrank(ranks, T):
    out = np.zeros((len(ranks), 4), np.int32)
    for i, r in enumerate(ranks):
        r, lo = int(r), 0
        for k in range(4, 0, -1):                   # the smallest remaining taxon whose block holds the rank
            t = lo
            while comb(T - t - 1, k - 1) <= r:
                r -= comb(T - t - 1, k - 1)
                t += 1
            out[i, 4 - k] = t
            lo = t + 1
    return out


def all_quartets(T):
    return np.array(list(combinations(range(T), 4)), np.int32).reshape(-1, 4)


def codes(parent, T, quartets):
    q = np.asarray(quartets)
    out = np.full(len(q), 3, np.int8)
    for side in dm.splits(parent, T):
        s = np.zeros(T, bool)
        s[list(side)] = True
        a, b, c, d = (s[q[:, k]] for k in range(4))
        out[(a == b) & (c == d) & (a != c)] = 0
        out[(a == c) & (b == d) & (a != b)] = 1
        out[(a == d) & (b == c) & (a != b)] = 2
    return out


def classes_of(code):
    """code i8 [N, Q] -> (A, B, C, D, E)."""
    N = len(code)
    res = code < 3
    out = [np.zeros((N, N), np.int64) for _ in range(5)]
    for i in range(N):
        eq = code == code[i]
        ri = res[i]
        out[0][i] = (ri & res & eq).sum(axis=1)
        out[1][i] = (ri & res & ~eq).sum(axis=1)
        out[2][i] = (ri & ~res).sum(axis=1)
        out[3][i] = (~ri & res).sum(axis=1)
        out[4][i] = (~ri & ~res).sum(axis=1)
    return tuple(out)


def expected(trees, T, quartets):
    code = np.stack([codes(p, T, quartets) for p in trees]) if len(trees) else np.zeros((0, len(quartets)), np.int8)
    return classes_of(code)


def sample_ranks(T, n, seed):
    return np.sort(np.random.default_rng(seed).choice(comb(T, 4), size=n, replace=False)).astype(np.uint64)


@lru_cache(maxsize=None)
def set_model(T, seed):
    trees = cm.tree_set(T, seed)
    if T <= FULL_T:
        ranks, quartets = None, all_quartets(T)
    else:
        ranks = sample_ranks(T, SAMPLE, seed)
        quartets = unrank(ranks, T)
    out = (trees, quartets, ranks) + expected(trees, T, quartets)
    for a in out[1:]:
        if a is not None:
            a.setflags(write=False)
    return out


def assert_matches(acc, classes, Q):
    A, B, C, D, E = classes
    got = acc.counts()
    for g, w in zip(got, classes):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w)
    np.testing.assert_array_equal(acc.distance(), B + C + D)
    np.testing.assert_array_equal(acc.resolved(), np.diag(A))
    assert acc.nquartets == Q and acc.ntrees == len(A)


def score_model(acc, quartets, ranks):
    """Scores the quartets of a `set_model` on `acc`: all of them, or the sampled ranks."""
    if ranks is None:
        acc.score_all()
    else:
        acc.score_ranks(ranks)


def nni_parts(t1, t2, T):
    """Two binary trees one NNI apart differ in one split each; the four subtrees around that edge are the four
    intersections of the two splits' sides.  Returns (sizes, the split of t1 that t2 lacks)."""
    s1, s2 = dm.splits(t1, T), dm.splits(t2, T)
    (x,), (y,) = s1 - s2, s2 - s1
    everyone = frozenset(range(T))
    parts = [x & y, x - y, y - x, everyone - x - y]
    assert all(parts) and sum(len(p) for p in parts) == T
    return [len(p) for p in parts], x


def contract(parent, T, side):
    """The tree without the internal edge whose split is `side`: the node below the edge hands its children to its
    parent and the nodes behind it move down by one."""
    parent = [int(p) for p in parent]
    below = [set() for _ in parent]
    for t in range(T):
        v = t
        while v >= 0:
            below[v].add(t)
            v = parent[v]
    everyone = set(range(T))
    gone = [v for v in range(T, len(parent)) if parent[v] >= 0 and (below[v] == set(side) or everyone - below[v] == set(side))]
    v = gone[0]
    up = parent[v]
    new = [up if p == v else p for p in parent]
    del new[v]
    return np.array([p - 1 if p > v else p for p in new], np.int32)
