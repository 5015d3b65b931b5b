"""Independent model of the quartet fit and tree builders for its tests.

The model works from the split definition alone: the taxa below every node of the parent array as Python int masks; a
tree displays p|q iff one of those masks holds pair p and misses pair q, or the other way round.  A row a,b|c,d is
satisfied when the tree displays ab|cd, violated when it displays ac|bd or ad|bc, unresolved otherwise.  No LCA table,
no depths; all sums are Python ints."""
import numpy as np

FIELDS = ("k_satisfied", "k_violated", "k_unresolved", "n_satisfied", "n_violated", "n_unresolved")


def side_masks(parent, T):
    """The set of taxa below every node, as Python ints (bit x = taxon x).  Trivial and repeated sides stay in: they
    separate no two pairs, or the same ones again."""
    parent = [int(p) for p in parent]
    n = len(parent)
    kids = [[] for _ in range(n)]
    root = None
    for v, p in enumerate(parent):
        if p < 0:
            root = v
        else:
            kids[p].append(v)
    order, stack = [], [root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(kids[v])
    assert len(order) == n, "not a tree"
    below = [0] * n
    for v in reversed(order):
        below[v] = (1 << v) if v < T else 0
        for c in kids[v]:
            below[v] |= below[c]
    assert below[root] == (1 << T) - 1, "a taxon is missing"
    return [below[v] for v in range(n) if v != root]


def taxon_memberships(masks, T):
    """S[x] = Python int whose bit e says that side e holds taxon x."""
    S = [0] * T
    for e, m in enumerate(masks):
        while m:
            low = m & -m
            S[low.bit_length() - 1] |= 1 << e
            m ^= low
    return S


def model_fit(parent, T, splits, k):
    """The six Python ints of one tree over rows splits[n,4] = a,b|c,d with integer weights k[n]."""
    S = taxon_memberships(side_masks(parent, T), T)

    def displays(p, q, r, s):
        return ((S[p] & S[q] & ~S[r] & ~S[s]) | (S[r] & S[s] & ~S[p] & ~S[q])) != 0

    out = [0] * 6
    for (a, b, c, d), w in zip(np.asarray(splits).tolist(), np.asarray(k).tolist()):
        sat = displays(a, b, c, d)
        vio = displays(a, c, b, d) or displays(a, d, b, c)
        assert not (sat and vio), "a tree cannot display two resolutions of one quartet"
        cls = 0 if sat else 1 if vio else 2
        out[cls] += int(w)
        out[3 + cls] += 1
    return out


def as_ints(rec):
    """A record of `Supertree.fit` as the model's list of six Python ints."""
    return [int(rec[f]) for f in FIELDS]


# -- tree builders (parent arrays: tips 0..T-1 = the taxa, internal nodes >= T, parent[root] = -1) ---------------------
def parent_from_children(children, root, T):
    n = T + len(children)
    ids = {v: v for v in range(T)}
    for i, v in enumerate(sorted(children)):
        ids[v] = T + i
    par = np.full(n, -1, np.int32)
    for p, cs in children.items():
        for c in cs:
            par[ids[c]] = ids[p]
    assert par[ids[root]] == -1
    return par


def star(T):
    return np.array([T] * T + [-1], np.int32)


def contract(parent, T, rng, frac=0.4):
    """The tree with about `frac` of its internal non-root nodes removed (their children move to the parent)."""
    par = [int(p) for p in parent]
    n = len(par)
    inner = [v for v in range(T, n) if par[v] >= 0]
    gone = set(v for v in inner if rng.random() < frac) or {inner[0]}
    out = list(par)
    for v in range(n):
        p = par[v]
        while p in gone:
            p = par[p]
        out[v] = p
    keep = [v for v in range(n) if v not in gone]
    new = {v: i for i, v in enumerate(keep)}
    return np.array([(-1 if out[v] < 0 else new[out[v]]) for v in keep], np.int32)


def reroot(parent, at):
    """The same unrooted tree hung from internal node `at` (the old root may be left with one child)."""
    par = np.array(parent, np.int32)
    path, v = [], int(at)
    while v >= 0:
        path.append(v)
        v = int(par[v])
    for child, up in zip(path[:-1], path[1:]):
        par[up] = child
    par[at] = -1
    return par


def subdivide(parent, edges):
    """A unary node on the edge above each node of `edges` (none of them the root)."""
    par = [int(p) for p in parent]
    for v in edges:
        assert par[v] >= 0
        par.append(par[v])
        par[v] = len(par) - 1
    return np.array(par, np.int32)


def root_on_edge(parent, v):
    """Re-rooted at a new degree-2 node in the middle of the edge above `v`."""
    par = subdivide(parent, [v])
    return reroot(par, len(par) - 1)
