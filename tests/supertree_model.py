"""Model and input builders for the exact supertree tests.  NumPy only: the root graph of
weighted splits by `np.add.at` on u64, generating trees of three shapes, and resolved rows made from a tree."""
import numpy as np

from tetrad_amd import synth

SUM_LIMIT = 1501199875790166          # smallest sum of k with 6 * sum >= 2^53


def model_graph(splits, k, T):
    """G (good edges a-c, a-d, b-c, b-d) and B (bad edges a-b, c-d) of splits u32[n,4] = a,b|c,d with integer weights
    k u64[n]: symmetric u64[T,T]."""
    sp = np.asarray(splits, np.int64).reshape(-1, 4)
    k = np.asarray(k, np.uint64)
    G = np.zeros((T, T), np.uint64)
    B = np.zeros((T, T), np.uint64)
    for M, pairs in ((B, [(0, 1), (2, 3)]), (G, [(0, 2), (0, 3), (1, 2), (1, 3)])):
        for i, j in pairs:
            np.add.at(M, (sp[:, i], sp[:, j]), k)
            np.add.at(M, (sp[:, j], sp[:, i]), k)
    return G, B


def tree_children(T, shape, rng):
    """(children, root) as synth.random_tree_children gives them: random joining, balanced, or caterpillar."""
    if shape == "random":
        return synth.random_tree_children(T, rng)
    children, nxt = {}, T
    if shape == "caterpillar":
        cur = 0
        for t in range(1, T):
            children[nxt] = (cur, t)
            cur, nxt = nxt, nxt + 1
        return children, cur
    assert shape == "balanced"
    layer = list(range(T))
    while len(layer) > 1:
        up = []
        for i in range(0, len(layer) - 1, 2):
            children[nxt] = (layer[i], layer[i + 1])
            up.append(nxt)
            nxt += 1
        if len(layer) % 2:
            up.append(layer[-1])
        layer = up
    return children, layer[0]


def tree_dist(children, root, T):
    """Pairwise path lengths between the tips (unit edges)."""
    parent = {}
    for p, (a, b) in children.items():
        parent[a] = parent[b] = p
    depth = {root: 0}
    order = [root]
    for v in order:
        for c in children.get(v, ()):
            depth[c] = depth[v] + 1
            order.append(c)
    anc = []
    for t in range(T):
        path, v = {}, t
        while True:
            path[v] = depth[v]
            if v == root:
                break
            v = parent[v]
        anc.append(path)
    D = np.zeros((T, T), np.int64)
    for i in range(T):
        for j in range(i + 1, T):
            v = j
            while v not in anc[i]:
                v = parent[v]
            D[i, j] = D[j, i] = depth[i] + depth[j] - 2 * depth[v]
    return D


def bipartitions(children, root, T):
    below, stack, post = {}, [root], []
    while stack:
        v = stack.pop()
        post.append(v)
        stack.extend(children.get(v, ()))
    for v in reversed(post):
        below[v] = frozenset([v]) if v < T else below[children[v][0]] | below[children[v][1]]
    allt = frozenset(range(T))
    return {min(s, allt - s, key=lambda x: (len(x), sorted(x))) for s in below.values() if 1 < len(s) < T - 1}


def newick_bipartitions(nwk, T):
    """Bipartitions of a newick with numeric tips; asserts that every taxon appears exactly once."""
    assert nwk.endswith(";")
    stack, splits, i, seen = [], [], 0, []
    while nwk[i] != ";":
        c = nwk[i]
        if c == "(":
            stack.append(None)
            i += 1
        elif c == ",":
            i += 1
        elif c == ")":
            s = frozenset()
            while stack[-1] is not None:
                s |= stack.pop()
            stack.pop()
            splits.append(s)
            stack.append(s)
            i += 1
        else:
            j = i
            while nwk[j].isdigit():
                j += 1
            seen.append(int(nwk[i:j]))
            stack.append(frozenset([seen[-1]]))
            i = j
    assert sorted(seen) == list(range(T)), "every taxon exactly once"
    allt = frozenset(range(T))
    return {min(s, allt - s, key=lambda x: (len(x), sorted(x))) for s in splits if 1 < len(s) < T - 1}


def true_topology(D, quartets):
    """Index of the tree's pairing of each quartet (0: ab|cd, 1: ac|bd, 2: ad|bc), the first smallest pair sum."""
    q = np.asarray(quartets, np.int64)
    a, b, c, d = q.T
    s = np.stack([D[a, b] + D[c, d], D[a, c] + D[b, d], D[a, d] + D[b, c]], axis=1)
    return np.argmin(s, axis=1).astype(np.uint32)


def sample_quartets(T, n, rng):
    """n random quartets (sorted taxa, repeats between rows allowed)."""
    q = np.empty((0, 4), np.int64)
    while len(q) < n:
        c = np.sort(rng.integers(0, T, size=(2 * n + 16, 4)), axis=1)
        c = c[(np.diff(c, axis=1) > 0).all(axis=1)]
        q = np.concatenate([q, c])
    return q[:n].astype(np.uint32)


def rows_from_tree(T, n, shape, wrong, seed, quartets=None):
    """Resolved rows of a generating tree: (children, root, quartets u32[n,4], rscor f64[n,3], rstat u32[n,2]).
    `wrong` of the rows carry one of the two other topologies; the chosen topology has the smallest score, the scores
    are multiples of 1/64 (exact under the 6-decimal rounding) so that every weight strategy sees varied weights."""
    rng = np.random.default_rng(seed)
    children, root = tree_children(T, shape, rng)
    D = tree_dist(children, root, T)
    q = sample_quartets(T, n, rng) if quartets is None else np.asarray(quartets, np.uint32)
    n = len(q)
    topo = true_topology(D, q)
    bad = rng.random(n) < wrong
    topo = np.where(bad, (topo + rng.integers(1, 3, n)) % 3, topo).astype(np.uint32)
    sc = rng.integers(2 * 64, 40 * 64, size=(n, 3)) / 64.0
    sc[np.arange(n), topo] = rng.integers(1, 2 * 64, n) / 64.0
    st = np.stack([topo, rng.integers(1, 3000, n).astype(np.uint32)], axis=1).astype(np.uint32)
    return children, root, q, sc, st


def bad_rows(T, n, rng):
    """Rows of every skipped kind: (quartets, rscor, rstat, flags)."""
    q = sample_quartets(T, n, rng)
    sc = rng.integers(64, 40 * 64, size=(n, 3)) / 64.0
    st = np.stack([rng.integers(0, 3, n), rng.integers(1, 3000, n)], axis=1).astype(np.uint32)
    fl = np.zeros(n, np.uint8)
    kind = np.arange(n) % 7
    q[kind == 0, 2] = T + np.arange((kind == 0).sum()) % 5            # taxon >= ntaxa
    q[kind == 1, 3] = q[kind == 1, 1]                                  # repeated taxon
    st[kind == 2, 0] = 3                                               # topology 3
    fl[kind == 3] = 4                                                  # TQ_FLAG_BAD_INDEX
    fl[kind == 4] = 16                                                 # TQ_FLAG_INVALID_DIAGNOSTIC
    st[kind == 5, 1] = 0                                               # zero-data row: no SNPs, zero scores
    sc[kind == 5] = 0.0
    fl[kind == 5] = 1
    sc[kind == 6] = [1e-6, 8.0e9, 8.0e9]                               # weight >= 4e9 under strategies 1 and 2
    return q, sc, st, fl
