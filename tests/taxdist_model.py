"""Independent model of the taxon counts and of neighbour joining.

Counts come straight from the u8 matrix with numpy comparisons (no bit planes); neighbour joining runs in plain Python
floats in the order the rule states; `splits` turns a parent array into taxon sets.
"""
import numpy as np


def tiling(S):
    """The cuts of tests/test_gpu_blocks.py: a tiling of [0, S) off and on the 32-site words (as far as S allows)."""
    cuts = sorted({c for c in (1, 5, 31, 32, 33, 64, 100, 129, 256, 300, 2047, 2048, 2049) if c < S})
    return np.array([0] + cuts + [S], np.int64)


def counts(tmparr, block_starts=None):
    """u32[B, T, T, 4] = (both, diff, ts, tv) per block."""
    a = np.asarray(tmparr)
    T, S = a.shape
    starts = [0, S] if block_starts is None else [int(v) for v in block_starts]
    out = np.zeros((len(starts) - 1, T, T, 4), np.uint32)
    for b in range(len(starts) - 1):
        x = a[:, starts[b]:starts[b + 1]].astype(np.int64)
        present = x <= 3
        for i in range(T):
            both = present[i][None, :] & present
            diff = both & (x[i][None, :] != x)
            lo, hi = np.minimum(x[i][None, :], x), np.maximum(x[i][None, :], x)
            ts = diff & (((lo == 0) & (hi == 2)) | ((lo == 1) & (hi == 3)))
            out[b, i, :, 0] = both.sum(axis=1)
            out[b, i, :, 1] = diff.sum(axis=1)
            out[b, i, :, 2] = ts.sum(axis=1)
            out[b, i, :, 3] = diff.sum(axis=1) - ts.sum(axis=1)
    return out


def nj(dist):
    """(parent list, length list) of d (T x T, nested lists or an array) in Python floats."""
    T = len(dist)
    d = {}
    for i in range(T):
        for j in range(T):
            if i != j:
                d[i, j] = float(dist[i][j])
    parent = [-1] * (2 * T - 2)
    length = [0.0] * (2 * T - 2)
    act = list(range(T))
    nxt = T
    while len(act) > 3:
        n = len(act)
        r = {}
        for i in act:
            s = 0.0
            for k in act:
                if k != i:
                    s = s + d[i, k]
            r[i] = s
        best = None
        for a in range(n):
            for b in range(a + 1, n):
                i, j = act[a], act[b]
                q = (float(n - 2) * d[i, j] - r[i]) - r[j]
                if best is None or q < best[0]:
                    best = (q, i, j)
        _, i, j = best
        u = nxt
        nxt += 1
        li = 0.5 * d[i, j] + (r[i] - r[j]) / (2.0 * float(n - 2))
        lj = d[i, j] - li
        parent[i] = parent[j] = u
        length[i], length[j] = li, lj
        for k in act:
            if k != i and k != j:
                d[u, k] = d[k, u] = 0.5 * ((d[i, k] + d[j, k]) - d[i, j])
        act = [k for k in act if k != i and k != j] + [u]
    i, j, k = act
    root = 2 * T - 3
    parent[i] = parent[j] = parent[k] = root
    length[i] = 0.5 * ((d[i, j] + d[i, k]) - d[j, k])
    length[j] = 0.5 * ((d[i, j] + d[j, k]) - d[i, k])
    length[k] = 0.5 * ((d[i, k] + d[j, k]) - d[i, j])
    return parent, length


def below(parent, T):
    """[node] -> frozenset of the taxa below it."""
    n = len(parent)
    sets = [set([v]) if v < T else set() for v in range(n)]
    order = sorted(range(n), key=lambda v: -depth(parent, v))
    for v in order:
        if parent[v] >= 0:
            sets[parent[v]] |= sets[v]
    return [frozenset(s) for s in sets]


def depth(parent, v):
    k = 0
    while parent[v] >= 0:
        v, k = parent[v], k + 1
    return k


def splits(parent, T):
    """The non-trivial splits of the unrooted tree as the set of the sides that do not hold taxon 0."""
    out = set()
    full = frozenset(range(T))
    for v, s in enumerate(below([int(p) for p in parent], T)):
        if parent[v] < 0:
            continue
        side = s if 0 not in s else full - s
        if 2 <= len(side) <= T - 2:
            out.add(side)
    return out


def split_lengths(parent, length, T):
    """{split: summed length of the edges that induce it} (a root of degree two puts two edges on one split)."""
    out = {}
    full = frozenset(range(T))
    for v, s in enumerate(below([int(p) for p in parent], T)):
        if parent[v] < 0:
            continue
        side = s if 0 not in s else full - s
        out[side] = out.get(side, 0.0) + float(length[v])
    return out


def children_to_parent(children, root, T):
    """The parent array of a `synth.random_tree_children` tree (internal nodes T..2T-2)."""
    parent = [-1] * (2 * T - 1)
    for v, (a, b) in children.items():
        parent[int(a)] = int(v)
        parent[int(b)] = int(v)
    assert parent[int(root)] == -1
    return parent
