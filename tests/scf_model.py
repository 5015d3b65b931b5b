"""An independent model of the site concordance accumulator, on Python integers.

The edge of a row and the tree's resolution r there come from `concordance_split_model.classify`: bipartition masks,
no LCA table, no depths, nothing `conc_build_tree` or `scf_row` compute.  The counts are Python integers and the
fixed-point share is `(x << 32) // inf`.  Edges are in the order of `split_masks`; `assert_matches` maps them to the
library's order through `library_order`.

    model = ScfModel(parent, T)
    model.add(sets, classes)            # any number of times
    model.words                         # [E][8] Python integers in the order of tetrad_amd.scf.WORDS
    assert_matches(acc, model)          # every word of acc.raw() bit for bit, and `skipped`

`class_rows` makes synthetic class rows with the values the fixed point has to survive; `scf_rows` puts rows aimed at
every edge (with at least one decisive site each) in front of mixed rows with bad taxa and rows without decisive sites.
"""
from __future__ import annotations

import numpy as np

from concordance_split_model import classify, library_order, mixed_rows, split_masks, targeted_rows

NQ, NQ_ZERO, SUM_CONC, SUM_D1, SUM_D2, FX_CONC, FX_D1, FX_D2 = range(8)
SUPPORT = (3, 6, 8)                    # classes 0011, 0101, 0110: the sites behind resolution 0, 1, 2 of the row
U32 = 2**32 - 1


def row_words(r, n):
    """(conc, d1, d2, fx_conc, fx_d1, fx_d2) of a row with resolution r and support counts n = (n0, n1, n2), or None
    when it has no decisive site."""
    inf = n[0] + n[1] + n[2]
    if inf == 0:
        return None
    lower, other = [k for k in range(3) if k != r]
    x = (n[r], n[lower], n[other])
    return x + tuple((v << 32) // inf for v in x)


class ScfModel:
    def __init__(self, parent, T):
        self.T = T
        self.masks = split_masks(parent, T)
        self.E = len(self.masks)
        self.words = [[0] * 8 for _ in range(self.E)]
        self.skipped = 0
        self.rows_induced = 0

    def add(self, sets, classes):
        q = np.asarray(sets).reshape(-1, 4).astype(np.int64)
        cl = np.asarray(classes).reshape(-1, 16)
        assert len(cl) == len(q)
        srt = np.sort(q, axis=1)
        bad = (srt[:, 1:] == srt[:, :-1]).any(1) | (q.max(1, initial=0) >= self.T)
        self.skipped += int(bad.sum())
        good = np.flatnonzero(~bad)
        edge, res = classify(self.masks, q[good])
        for i, e, r in zip(good[edge >= 0].tolist(), edge[edge >= 0].tolist(), res[edge >= 0].tolist()):
            self.rows_induced += 1
            w = self.words[e]
            x = row_words(r, tuple(int(cl[i, k]) for k in SUPPORT))
            if x is None:
                w[NQ_ZERO] += 1
                continue
            w[NQ] += 1
            for k in range(6):
                w[SUM_CONC + k] += x[k]


def assert_matches(acc, model):
    """Every word of the accumulator against the model, as Python integers.  Returns (idx, words of the library in
    the model's edge order)."""
    idx = library_order(acc, model.masks)
    raw = acc.raw()
    assert raw["edge_counts"].dtype == np.uint64 and raw["edge_counts"].shape == (model.E, 8)
    got = [[int(x) for x in row] for row in raw["edge_counts"][idx]]
    assert got == model.words
    assert raw["skipped"] == model.skipped
    return idx, got


# -- rows ----------------------------------------------------------------------------------------------------------
def class_rows(n, rng, decisive=False):
    """u32[n,16] synthetic class rows: random counts in every slot (slot 15 holds noise: it must not be read), and
    among the three support classes counts of 2^32 - 1 in one, two and all three, ties n0 = n1 = n2, single non-zero
    classes and -- unless `decisive` -- rows whose three support classes are all zero."""
    c = rng.integers(0, 3000, size=(n, 16)).astype(np.uint32)
    c[:, 15] = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    k = rng.random(n)
    s = np.array(SUPPORT)

    def put(sel, values):
        rows = np.flatnonzero(sel)
        c[rows[:, None], s[None, :]] = np.asarray(values, np.uint32)

    one = rng.integers(0, 3, n)
    big1 = np.where(np.arange(3)[None, :] == one[:, None], U32, c[:, s])
    big2 = np.where(np.arange(3)[None, :] != one[:, None], U32, c[:, s])
    put(k < 0.04, big1[k < 0.04])
    put((k >= 0.04) & (k < 0.08), big2[(k >= 0.04) & (k < 0.08)])
    put((k >= 0.08) & (k < 0.12), U32)
    tie = (k >= 0.12) & (k < 0.18)
    put(tie, np.repeat(rng.integers(1, 5000, size=(int(tie.sum()), 1)), 3, axis=1))
    only = (k >= 0.18) & (k < 0.24)
    put(only, np.where(np.arange(3)[None, :] == one[only][:, None], c[only][:, s] + 1, 0))
    zero = (k >= 0.24) & (k < 0.32)
    put(zero, np.ones((int(zero.sum()), 3), np.uint32) if decisive else 0)
    if decisive:
        c[(c[:, s] == 0).all(1), 3] = 1
    return c


def scf_rows(model, k, n_mixed, rng, window=None, family=None):
    """(sets u32[m,4], classes u32[m,16]): k rows aimed at every edge, each with a decisive site, then `n_mixed`
    random rows (unsorted positions, repeated and out-of-range taxa) with every kind of class row."""
    tq, target = targeted_rows(model.masks, model.T, k, rng, family=family)
    assert np.array_equal(np.bincount(target, minlength=model.E), np.full(model.E, k))
    mq = mixed_rows(model.T, n_mixed, rng, window=window)[0]
    sets = np.concatenate([tq.astype(np.uint32), mq]).astype(np.uint32)
    classes = np.concatenate([class_rows(len(tq), rng, decisive=True), class_rows(n_mixed, rng)])
    return np.ascontiguousarray(sets), np.ascontiguousarray(classes)
