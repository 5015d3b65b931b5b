"""A second model of the concordance accumulator, one that scales to T = 4096 ("tested range").

`concordance_model.ConcordanceModel` enumerates every quartet the tree induces, so it stops at about T = 40.  This one
works from the bipartitions of the tree alone: no LCA table, no depths, no edge numbering, nothing the library's
`conc_build_tree` / `conc_row` compute.

    masks = split_masks(parent, T)                  # bool [E, T], the side without taxon 0, sorted, no duplicates
    edge, res = classify(masks, q)                  # per row: the one edge that separates it 2|2 (or -1), the
                                                    # tree's resolution in the row's own positions
    model = SplitModel(parent, T, min_snps, min_ratio)
    model.add(q, rscor, rstat, flags)               # any number of times
    model.result()                                  # arrays in the order of model.masks; float sums by math.fsum
    targeted_rows(masks, T, k, rng)                 # k rows induced on every edge (checked by `classify`)

Row rule: an edge separates a row 2|2 when exactly two of its four taxa lie on the edge's side.  Walking the path
between the two pairs of a resolved quartet, every edge of that path separates it 2|2, so the row is induced on an
edge (internal path one edge long) iff exactly one edge does.
"""
from __future__ import annotations

from math import fsum

import numpy as np

from concordance_model import reread6, row_values


# -- trees -------------------------------------------------------------------------------------------------------------
def caterpillar(T):
    """Parent array of the caterpillar ((((0,1),2),3),...,T-1): a degree-2 root, depth T - 1."""
    parent = [-1] * T
    prev = 0
    for t in range(1, T):
        v = len(parent)
        parent.append(-1)
        parent[prev] = v
        parent[t] = v
        prev = v
    return np.array(parent, np.int32)


def collapse_clade(parent, T, share=0.3):
    """The parent array with one clade of about `share` of the taxa collapsed into a polytomy: every tip below the
    chosen node becomes its child, the internal nodes below it are removed (nodes renumbered, taxa keep 0..T-1)."""
    parent = np.asarray(parent)
    n = len(parent)
    ntips = np.zeros(n, np.int64)
    ntips[:T] = 1
    order = _preorder(parent)
    for v in reversed(order):
        if parent[v] >= 0:
            ntips[parent[v]] += ntips[v]
    cand = np.arange(T, n)
    v0 = int(cand[np.argmin(np.abs(ntips[T:] - share * T))])
    top = np.full(n, False)                       # strictly below v0
    for v in order:
        if parent[v] >= 0 and (parent[v] == v0 or top[parent[v]]):
            top[v] = True
    keep = [v for v in range(n) if v < T or not top[v]]
    new = {v: i for i, v in enumerate(keep)}
    out = np.full(len(keep), -1, np.int32)
    for v in keep:
        p = v0 if top[v] else parent[v]
        out[new[v]] = -1 if p < 0 else new[int(p)]
    return out


def _preorder(parent):
    n = len(parent)
    kids = [[] for _ in range(n)]
    root = -1
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
    assert len(order) == n
    return order


# -- splits ------------------------------------------------------------------------------------------------------------
def split_masks(parent, T):
    """bool [E, T]: for every node, the taxa below it, normalised to the side without taxon 0; sides of fewer than 2
    or more than T - 2 taxa dropped; duplicates (unary chains, the two edges at a degree-2 root) removed."""
    parent = np.asarray(parent)
    n = len(parent)
    below = np.zeros((n, T), bool)
    below[np.arange(T), np.arange(T)] = True
    for v in reversed(_preorder(parent)):
        if parent[v] >= 0:
            below[parent[v]] |= below[v]
    m = below[T:]
    m = np.where(m[:, :1], ~m, m)
    size = m.sum(1)
    m = m[(size >= 2) & (size <= T - 2)]
    return np.unique(m, axis=0)


def classify(masks, q, chunk=2000):
    """Per row of q (four distinct taxa < T each): the index of the only edge that separates it 2|2, or -1 when none
    or several do; and the tree's resolution r = 0 / 1 / 2 (position 0 shares its side with position 1 / 2 / 3)."""
    q = np.asarray(q, np.int64).reshape(-1, 4)
    n = len(q)
    edge = np.full(n, -1, np.int64)
    res = np.full(n, -1, np.int64)
    if not len(masks) or not n:
        return edge, res
    by_taxon = np.ascontiguousarray(masks.T).view(np.uint8)          # [T, E]
    for i in range(0, n, chunk):
        x = by_taxon[q[i:i + chunk]]                                  # [c, 4, E]
        two = x.sum(1, dtype=np.uint8) == 2                          # [c, E]
        e = two.argmax(1)
        ok = two.sum(1) == 1
        xe = x[np.arange(len(e)), :, e]                               # [c, 4]
        r = np.where(xe[:, 0] == xe[:, 1], 0, np.where(xe[:, 0] == xe[:, 2], 1, 2))
        edge[i:i + chunk] = np.where(ok, e, -1)
        res[i:i + chunk] = np.where(ok, r, -1)
    return edge, res


class CladeFamily:
    """The normalised sides are a laminar family: the clades of the tree rooted at taxon 0.  `par[e]` is the smallest
    clade strictly holding clade e (index E = the root clade, every taxon but 0); the parts of a clade are its child
    clades plus its leftover single tips."""

    def __init__(self, masks, T):
        self.masks, self.T = masks, T
        E = self.E = len(masks)
        self.size = np.append(masks.sum(1), T - 1).astype(np.int64)
        order = np.argsort(self.size[:E], kind="stable")
        ms, ss = masks[order], self.size[:E][order]
        self.par = np.full(E, E, np.int64)
        for i in range(E):
            t = int(np.flatnonzero(ms[i])[0])
            bigger = np.flatnonzero(ms[i + 1:, t] & (ss[i + 1:] > ss[i]))
            if len(bigger):
                self.par[order[i]] = order[i + 1 + bigger[0]]
        self.kids = [[] for _ in range(E + 1)]
        for e in range(E):
            self.kids[self.par[e]].append(e)

    def mask(self, e):
        if e == self.E:
            full = np.ones(self.T, bool)
            full[0] = False
            return full
        return self.masks[e]

    def parts(self, e):
        """Taxa of each part of clade e (child clades first, then the leftover tips)."""
        left = self.mask(e).copy()
        out = []
        for c in self.kids[e]:
            out.append(np.flatnonzero(self.masks[c]))
            left &= ~self.masks[c]
        return out + [np.array([t]) for t in np.flatnonzero(left)]

    def part_sizes(self, e, without=None):
        s = [int(self.size[c]) for c in self.kids[e]]
        left = int(self.size[e]) - sum(s)
        assert left >= 0
        if without is not None:
            s.remove(int(self.size[without]))
        return s + [1] * left

    def nqrts(self):
        """Quartets each edge induces: (pairs of parts below) x (pairs of parts at the far end), Python integers."""
        def pairs(s):
            a, b = sum(s), sum(x * x for x in s)
            return (a * a - b) // 2
        out = []
        for e in range(self.E):
            p = int(self.par[e])
            above = self.part_sizes(p, without=e) + [self.T - int(self.size[p])]
            out.append(pairs(self.part_sizes(e)) * pairs(above))
        return out


def targeted_rows(masks, T, k, rng, family=None):
    """(rows i64[k E, 4], target i64[k E]): k rows induced on every edge.  a and b come from two different parts of
    the edge's clade, c and d from two different parts at the far end (the clade's siblings, or the complement of the
    parent clade); the four positions are permuted.  Every row is classified by the row rule and must come out on
    its target edge."""
    fam = family or CladeFamily(masks, T)
    E = fam.E
    parts = [fam.parts(e) for e in range(E + 1)]
    rows, target = [], []
    for e in range(E):
        below = parts[e]
        p = int(fam.par[e])
        above = [x for x in parts[p] if not masks[e][x[0]]] + [np.flatnonzero(~fam.mask(p))]
        assert len(below) >= 2 and len(above) >= 2
        for _ in range(k):
            i, j = rng.choice(len(below), 2, replace=False)
            u, v = rng.choice(len(above), 2, replace=False)
            r = [rng.choice(below[i]), rng.choice(below[j]), rng.choice(above[u]), rng.choice(above[v])]
            rows.append(rng.permutation(r))
            target.append(e)
    rows = np.array(rows, np.int64).reshape(-1, 4)
    target = np.array(target, np.int64)
    edge, _ = classify(masks, rows)
    assert np.array_equal(edge, target), "targeted_rows: a generated row is not induced on its target edge"
    return rows, target


# -- rows --------------------------------------------------------------------------------------------------------------
def mixed_rows(T, n, rng, window=None):
    """Random rows with the mix of tests/test_gpu_concordance.py::rows: unsorted positions, every flag, repeated and
    out-of-range taxa, a topology > 2, 6-decimal rounding ties, scores on the min_ratio = 1.25 boundary, all-zero
    scores.  `window`: the four taxa of a row come from that many neighbouring taxa (for a caterpillar, where four
    taxa drawn from the whole tree are hardly ever one edge apart)."""
    if window:
        start = rng.integers(0, T - window + 1, n)
        off = np.argsort(rng.random((n, window)), axis=1)[:, :4]
        q = (start[:, None] + off).astype(np.uint32)
    else:
        q = rng.integers(0, T, size=(n, 4)).astype(np.uint32)         # a few repeat a taxon (skipped)
    sc = rng.uniform(0.0, 400.0, size=(n, 3))
    k = rng.random(n)
    sc[k < 0.1] = rng.integers(0, 400 * 128, size=(int((k < 0.1).sum()), 3)) / 128.0      # 6-decimal ties
    b = (k >= 0.1) & (k < 0.2)
    sc[b] = np.array([1.0, 1.25, 1.25]) * rng.integers(1, 100, size=(int(b.sum()), 1))      # score == 1.25 exactly
    sc[(k >= 0.2) & (k < 0.22)] = 0.0
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 40, n)], axis=1).astype(np.uint32)
    fl = np.zeros(n, np.uint8)
    m = rng.random(n)
    fl[m < 0.05] = rng.choice([1, 2, 4, 8, 16], size=int((m < 0.05).sum()))
    q[(m >= 0.05) & (m < 0.06), 3] = q[(m >= 0.05) & (m < 0.06), 0]
    q[(m >= 0.06) & (m < 0.07), 1] = T + 3
    st[(m >= 0.07) & (m < 0.075), 0] = 3
    return q, sc, st, fl


def dress_rows(q, rng):
    """Scores, topology / nsnps and flags for given quartets (the targeted rows): mostly countable, with the same
    kinds of ties and boundary scores as `mixed_rows`, no bad rows."""
    n = len(q)
    _, sc, st, _ = mixed_rows(8, n, rng)
    st[:, 0] = rng.integers(0, 3, n)
    return np.ascontiguousarray(q, dtype=np.uint32), sc, st, np.zeros(n, np.uint8)


# -- the accumulator ---------------------------------------------------------------------------------------------------
class SplitModel:
    """`ConcordanceModel.add` restated on split masks: the same skip rule, thresholds, classes, weight and score."""

    def __init__(self, parent, T, min_snps=0, min_ratio=1.0):
        self.T = T
        self.min_snps = max(1, int(min_snps))          # deviation 2
        self.min_ratio = float(min_ratio)
        self.masks = split_masks(parent, T)
        self.family = CladeFamily(self.masks, T)
        E = self.E = len(self.masks)
        self.counts = np.zeros((E, 4), np.int64)        # conc, disc1, disc2, nu
        self.nsnps = [0] * E                            # Python integers
        self.weights = [[] for _ in range(E)]
        self.scores = [[] for _ in range(E)]
        self.QFc = np.zeros(T, np.int64)
        self.QFd = np.zeros(T, np.int64)
        self.skipped = 0
        self.rows_seen = 0
        self.rows_induced = 0

    def add(self, quartets, rscor, rstat, flags=None):
        q = np.asarray(quartets).reshape(-1, 4).astype(np.int64)
        st = np.asarray(rstat).reshape(-1, 2).astype(np.int64)
        sc = np.asarray(rscor, np.float64).reshape(-1, 3)
        n = len(q)
        fl = np.zeros(n, np.int64) if flags is None else np.asarray(flags).astype(np.int64)
        srt = np.sort(q, axis=1)
        bad = ((fl & (4 | 16)) != 0) | (srt[:, 1:] == srt[:, :-1]).any(1) | (q.max(1) >= self.T) | (st[:, 0] > 2)
        self.skipped += int(bad.sum())
        self.rows_seen += n
        good = np.flatnonzero(~bad)
        edge, res = classify(self.masks, q[good])
        for i, e, r in zip(good[edge >= 0], edge[edge >= 0], res[edge >= 0]):
            self.rows_induced += 1
            rhat, nsnps = int(st[i, 0]), int(st[i, 1])
            weight, score = row_values(sc[i])
            self.nsnps[e] += nsnps
            self.weights[e].append(weight)
            self.scores[e].append(score)
            if score < self.min_ratio or nsnps < self.min_snps:
                self.counts[e, 3] += 1
                continue
            if rhat == r:
                self.counts[e, 0] += 1
                self.QFc[q[i]] += 1
            else:
                self.QFd[q[i]] += 1
                lower = min(k for k in range(3) if k != r)
                self.counts[e, 1 if rhat == lower else 2] += 1

    def result(self):
        c = self.counts
        with np.errstate(invalid="ignore", divide="ignore"):
            qf = np.where(self.QFc + self.QFd > 0, self.QFc / (self.QFc + self.QFd), np.nan)
        return dict(masks=self.masks, nqrts=self.family.nqrts(), conc=c[:, 0].copy(), disc1=c[:, 1].copy(),
                    disc2=c[:, 2].copy(), nu=c[:, 3].copy(), counted=c.sum(1), nsnps_sum=list(self.nsnps),
                    weight_sum=np.array([fsum(w) for w in self.weights]),
                    score_sum=np.array([fsum(s) for s in self.scores]),
                    QFc=self.QFc.copy(), QFd=self.QFd.copy(), QF=qf, skipped=self.skipped)


def library_order(acc, masks):
    """idx with masks[e] == the library's edge idx[e] (through `stats()["split"]`, normalised to the side without
    taxon 0); asserts that the two edge sets are the same."""
    lib = acc.split_masks()
    lib = np.where(lib[:, :1], ~lib, lib)
    assert len(lib) == len(masks), (len(lib), len(masks))
    key = {np.packbits(m).tobytes(): i for i, m in enumerate(lib)}
    assert len(key) == len(lib), "the library reports one split twice"
    idx = np.array([key.get(np.packbits(m).tobytes(), -1) for m in masks], np.int64)
    assert (idx >= 0).all(), "a split of the model is missing in the library"
    return idx


def assert_raw_matches(acc, model, rel=1e-12):
    """The accumulator's raw counters against the split model: integer words exactly, weight / score sums within
    `rel` of the fsum."""
    res = model.result()
    idx = library_order(acc, res["masks"])
    raw = acc.raw()
    c = raw["edge_counts"][idx]
    assert [int(x) for x in c[:, 0]] == res["nqrts"]
    for j, k in enumerate(("conc", "disc1", "disc2", "nu"), 1):
        np.testing.assert_array_equal(c[:, j], res[k], err_msg=k)
    assert [int(x) for x in c[:, 5]] == res["nsnps_sum"]
    np.testing.assert_array_equal(raw["tip_counts"][:, 0], res["QFc"])
    np.testing.assert_array_equal(raw["tip_counts"][:, 1], res["QFd"])
    assert raw["skipped"] == res["skipped"]
    np.testing.assert_allclose(raw["edge_sums"][idx, 0], res["weight_sum"], rtol=rel, atol=0)
    np.testing.assert_allclose(raw["edge_sums"][idx, 1], res["score_sum"], rtol=rel, atol=0)
    return idx, raw, res
