"""An independent model of the transfer bootstrap accumulator, written from the rule alone.

Sides are Python `frozenset`s of taxa from a traversal of its own: no bit masks, no popcount, no library call.

    edge_sides(parent, T)        # one frozenset per edge of the tree, the edges above tips included
    each_edge_side(parent, T)    # the same, one at a time (large trees)
    delta(A, B, T)               # min(|A xor B|, T - |A xor B|)
    branches(parent, T)          # the reference branches in accumulator order, with p
    phi(branch, sides, T)        # the minimum of delta over EVERY edge -- no clamp to p - 1: that the accumulator's
                                 # clamped minimum over the internal nodes is the same thing is what the tests show
    expected(ref, trees, T)      # (masks bool[E, T], p i64[E], phi i64[R, E])
    percent(phi_sum, p, ntrees)  # the integer label

`set_model(T, seed, ref)` is the model of the 40 trees of `consensus_model.tree_set(T, seed)` against tree number `ref`
of that set, computed once per process and shared by the tests; callers leave its arrays unchanged.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import consensus_model as cm


def each_edge_side(parent, T):
    """The taxa below every non-root node, one after the other (only the sides still to be joined are kept alive)."""
    parent = [int(p) for p in parent]
    kids = cm.kids_of(parent)
    root = parent.index(-1)
    order = [root]
    for v in order:
        order.extend(kids[v])
    below = {}
    for v in reversed(order):
        below[v] = frozenset([v]) if v < T else frozenset().union(*(below.pop(k) for k in kids[v]))
        if v != root:
            yield below[v]


def edge_sides(parent, T):
    """The set of them (unary nodes and a degree-2 root repeat a side; a set holds it once)."""
    return set(each_edge_side(parent, T))


def delta(A, B, T):
    d = len(A ^ B)
    return min(d, T - d)


def branches(parent, T):
    """[(side without taxon 0, p)] ordered as the accumulator orders them: the side ascending as the sum of 2^taxon."""
    sides = sorted(cm.splits_of(parent, T), key=lambda s: sorted(s, reverse=True))
    return [(s, min(len(s), T - len(s))) for s in sides]


def phi(branch, sides, T):
    return min(delta(branch, s, T) for s in sides)


_PHI = {}       # (T, branch, frozenset of sides) -> phi: trees of one set share most of their branches


def expected(ref, trees, T, sides=None):
    br = branches(ref, T)
    if sides is None:
        sides = [frozenset(edge_sides(t, T)) for t in trees]
    masks = np.zeros((len(br), T), bool)
    for e, (s, _) in enumerate(br):
        masks[e, sorted(s)] = True
    out = np.zeros((len(trees), len(br)), np.int64)
    for r, ss in enumerate(sides):
        for e, (s, _) in enumerate(br):
            key = (T, s, ss)
            if key not in _PHI:
                _PHI[key] = phi(s, ss, T)
            out[r, e] = _PHI[key]
    return masks, np.array([p for _, p in br], np.int64), out


@lru_cache(maxsize=None)
def _set(T, seed):
    trees = cm.tree_set(T, seed)
    return trees, [frozenset(edge_sides(t, T)) for t in trees]


@lru_cache(maxsize=None)
def set_model(T, seed, ref):
    """(trees, masks, p, phi) of `tree_set(T, seed)` against its tree number `ref`."""
    trees, sides = _set(T, seed)
    return (trees,) + expected(trees[ref], trees, T, sides)


def percent(phi_sum, p, ntrees):
    """1 - phi_sum / (ntrees (p - 1)) as a percent rounded half up, from a doubled numerator (no library formula)."""
    nq = ntrees * (p - 1)
    twice = 2 * 100 * (nq - phi_sum)            # twice the percent, times nq
    return (twice + nq) // (2 * nq)


def newick_of(parent, T):
    """Newick text of a parent array (numeric tips), children in node order."""
    kids = cm.kids_of(parent)
    root = [int(p) for p in parent].index(-1)
    order = [root]
    for v in order:
        order.extend(kids[v])
    text = {}
    for v in reversed(order):
        text[v] = str(v) if v < T else "(" + ",".join(text.pop(k) for k in kids[v]) + ")"
    return text[root] + ";"


def assert_matches(acc, masks, p, phi_rows):
    """The accumulator's `raw()` against the model's rows of the trees it was given."""
    got_masks, got_p, got_sum = acc.raw()
    np.testing.assert_array_equal(got_masks, masks)
    np.testing.assert_array_equal(got_p, p)
    np.testing.assert_array_equal(got_sum.astype(np.int64), phi_rows.sum(axis=0))
    assert acc.ntrees == len(phi_rows)
