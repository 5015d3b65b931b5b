"""An independent model of the consensus accumulator, written from the definitions alone.

Splits are Python `frozenset`s of taxa computed from parent arrays by a traversal of its own: no bit masks, no library
call, nothing `conc_build_tree` / `cons_prepare` compute.  A degree-2 root and unary nodes need no special handling
here: the two edges they join give the same set, and a set holds it once.

    splits_of(parent, T)                        # set of frozensets: the side without taxon 0, 2 <= size <= T - 2
    table(list of split sets)                   # [(frozenset, count)] in canonical order
    min_count(min_freq, ntrees)                 # the integer threshold
    consensus(table, T, ntrees, min_count)      # newick with integer percent supports
    table_arrays(table, T)                      # (bool [n, T], i64 [n]) to compare with `Consensus.splits()`

Generators (parent arrays, tips 0..T-1): balanced, caterpillar, random_binary, multifurcating, unrooted (degree-3
root), with_unary, star, nni (a random nearest-neighbour interchange), and `tree_set`: 10 base shapes x 4 perturbations.
"""
from __future__ import annotations

from collections import Counter, defaultdict
from decimal import Decimal

import numpy as np

from concordance_split_model import caterpillar, collapse_clade  # noqa: F401  (caterpillar is re-exported)
from supertree_model import tree_children


# -- trees -------------------------------------------------------------------------------------------------------------
def children_to_parent(children, root, T):
    """(children dict, root) of supertree_model -> parent array with internal nodes renumbered T.."""
    ids = {v: i for i, v in enumerate(sorted(children), start=T)}
    parent = np.full(T + len(children), -1, np.int32)
    for p, kids in children.items():
        for c in kids:
            parent[c if c < T else ids[c]] = ids[p]
    assert parent[ids[root]] == -1
    return parent


def balanced(T):
    return children_to_parent(*tree_children(T, "balanced", None), T)


def random_binary(T, rng):
    return children_to_parent(*tree_children(T, "random", rng), T)


def multifurcating(T, rng, share=0.3):
    return collapse_clade(random_binary(T, rng), T, share)


def star(T):
    return np.array([T] * T + [-1], np.int32)


def kids_of(parent):
    kids = defaultdict(list)
    for v, p in enumerate(parent):
        if p >= 0:
            kids[int(p)].append(v)
    return kids


def unrooted(parent, T):
    """The same tree with its degree-2 root dissolved (the root's internal child becomes the root)."""
    parent = np.array(parent, np.int32)
    root = int(np.flatnonzero(parent < 0)[0])
    kids = kids_of(parent)[root]
    if len(kids) != 2:
        return parent
    a, b = kids if kids[0] >= T else kids[::-1]
    assert a >= T
    parent[b] = a
    parent[a] = -1
    keep = [v for v in range(len(parent)) if v != root]
    new = {v: i for i, v in enumerate(keep)}
    return np.array([-1 if parent[v] < 0 else new[int(parent[v])] for v in keep], np.int32)


def with_unary(parent, T, rng, k=3):
    """k unary nodes put on random edges (one above the root among them)."""
    parent = [int(p) for p in parent]
    for i in range(k):
        v = parent.index(-1) if i == 0 else int(rng.integers(0, len(parent)))
        u = len(parent)
        parent.append(parent[v])
        parent[v] = u
    return np.array(parent, np.int32)


def nni(parent, T, rng):
    """One nearest-neighbour interchange over a random internal edge (u, v): a child of v trades places with a sibling
    of v.  A tree without an internal edge comes back unchanged."""
    parent = np.array(parent, np.int32)
    kids = kids_of(parent)
    edges = [v for v in range(T, len(parent)) if parent[v] >= 0 and len(kids[int(parent[v])]) >= 2 and len(kids[v]) >= 2]
    if not edges:
        return parent
    v = int(edges[rng.integers(0, len(edges))])
    u = int(parent[v])
    sib = [s for s in kids[u] if s != v]
    c = kids[v][rng.integers(0, len(kids[v]))]
    s = sib[rng.integers(0, len(sib))]
    parent[c], parent[s] = u, v
    return parent


def tree_set(T, seed):
    """40 trees: 10 base shapes (a random binary tree, that tree unrooted, with unary nodes, after 1 / 3 / 6 NNIs, with
    a clade collapsed into a polytomy, a balanced tree, a caterpillar, a star) x 4 perturbations (itself, then 1, 2 and
    3 further NNIs), so that the counts spread between 1 and 40."""
    rng = np.random.default_rng(seed)
    base = random_binary(T, rng)
    moved = [base]
    for _ in range(6):
        moved.append(nni(moved[-1], T, rng))
    bases = [base, unrooted(base, T), with_unary(base, T, rng), moved[1], moved[3], moved[6],
             collapse_clade(base, T, 0.3), balanced(T), caterpillar(T), star(T)]
    out = []
    for b in bases:
        t = b
        out.append(t)
        for _ in range(3):
            t = nni(t, T, rng)
            out.append(t)
    return out


# -- the model ---------------------------------------------------------------------------------------------------------
def splits_of(parent, T):
    """The splits of a tree: for every node the taxa below it, taken as the side without taxon 0; sides of fewer than 2
    or more than T - 2 taxa are no splits."""
    parent = [int(p) for p in parent]
    n = len(parent)
    kids = kids_of(parent)
    assert all(not kids[t] for t in range(T)) and all(kids[v] for v in range(T, n)), "taxa are exactly the tips"
    root = parent.index(-1)
    order = [root]
    for v in order:
        order.extend(kids[v])
    assert len(order) == n
    below = {}
    everyone = frozenset(range(T))
    out = set()
    for v in reversed(order):
        below[v] = frozenset([v]) if v < T else frozenset().union(*(below.pop(k) for k in kids[v]))
        side = everyone - below[v] if 0 in below[v] else below[v]
        if 2 <= len(side) <= T - 2:
            out.add(side)
    return out


def order_key(item):
    """Canonical order: count descending, then the side ascending as the integer sum of 2^taxon.  Of two different
    sides the larger integer is the one that holds the largest taxon they do not share, which is the lexicographic order
    of the taxa listed downwards."""
    side, count = item
    return (-count, sorted(side, reverse=True))


def table(split_sets):
    counts = Counter()
    for s in split_sets:
        counts.update(s)
    return sorted(counts.items(), key=order_key)


def min_count(min_freq, ntrees):
    """max(1, ceil(min_freq x ntrees)) with min_freq read as its shortest decimal text; 0.5 asks for a strict majority."""
    num, den = Decimal(repr(float(min_freq))).as_integer_ratio()
    k = max(1, -((-num * ntrees) // den))
    if min_freq == 0.5:
        while 2 * k <= ntrees:
            k += 1
    return k


def compatible(a, b):
    return a.isdisjoint(b) or a <= b or b <= a


def accepted(tab, mincount):
    acc = []
    for side, count in tab:
        if count >= mincount and all(compatible(side, other) for other, _ in acc):
            acc.append((side, count))
    return acc


def percent(count, ntrees):
    return (200 * count + ntrees) // (2 * ntrees)


def consensus(tab, T, ntrees, mincount):
    """The consensus newick: the accepted sides nest; the root holds the maximal sides and the uncovered tips, children
    are ordered by their smallest taxon, an accepted side carries its integer percent."""
    acc = accepted(tab, mincount)
    holding = defaultdict(list)                 # taxon -> accepted sides that hold it (a chain, since they nest)
    for i, (side, _) in enumerate(acc):
        for x in side:
            holding[x].append(i)
    kids = defaultdict(list)                    # index of a side, or -1 for the root -> children (smallest taxon, text or index)
    for i, (side, _) in enumerate(acc):
        bigger = [j for j in holding[min(side)] if len(acc[j][0]) > len(side)]
        up = min(bigger, key=lambda j: len(acc[j][0])) if bigger else -1
        kids[up].append((min(side), i))
    for x in range(T):
        chain = holding[x]
        up = min(chain, key=lambda j: len(acc[j][0])) if chain else -1
        kids[up].append((x, str(x)))
    text = {}
    for i in sorted(range(len(acc)), key=lambda j: len(acc[j][0])):      # small sides first: children before parents
        parts = [c if isinstance(c, str) else text.pop(c) for _, c in sorted(kids[i], key=lambda p: p[0])]
        text[i] = "(" + ",".join(parts) + ")" + str(percent(acc[i][1], ntrees))
    parts = [c if isinstance(c, str) else text.pop(c) for _, c in sorted(kids[-1], key=lambda p: p[0])]
    return "(" + ",".join(parts) + ");"


def table_arrays(tab, T):
    masks = np.zeros((len(tab), T), bool)
    for i, (side, _) in enumerate(tab):
        masks[i, sorted(side)] = True
    return masks, np.array([c for _, c in tab], np.int64)


def model_of(trees, T):
    """(table, ntrees) of a list of parent arrays."""
    return table([splits_of(p, T) for p in trees]), len(trees)


def assert_matches(acc, tab, ntrees, T):
    """The accumulator's table against the model's: same splits, same counts, same order."""
    masks, counts, n = acc.splits()
    want_masks, want_counts = table_arrays(tab, T)
    assert n == ntrees
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(masks, want_masks)
