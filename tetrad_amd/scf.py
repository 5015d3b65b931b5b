"""Site concordance factors per branch of a fixed tree: IQ-TREE's sCF / sDF1 / sDF2 / sN (Minh, Hahn & Lanfear 2020),
the site-level companion of the quartet-level QC / QD / QI of `concordance.Concordance`.

For a quartet of taxa around a branch, the decisive sites are those of the three two-by-two patterns: class 3 (`0011`),
class 6 (`0101`) and class 8 (`0110`) of its class row (`patterns.CLASS_STRINGS`).  One of the three agrees with the
branch.  The share of the decisive sites that agrees, averaged over the quartets of the branch, is its sCF; the two
other shares are sDF1 and sDF2, and the mean number of decisive sites is sN.

The rows are counted by the library (`tq_scf_*`, tetrad_amd/csrc/scf.hpp) on the tree machinery of the concordance
accumulator: on host arrays (`SiteConcordance.add`, no device needed) or on device arrays right where
`QuartetEngine.patterns_dev` wrote them (`SiteConcordance.add_dev`, a HIP kernel, asynchronous).  Per edge the library
keeps eight unsigned 64-bit sums:

    nq, nq_zero                     rows with and without a decisive site
    sum_conc, sum_d1, sum_d2        decisive sites that agree / support the lower / the other remaining resolution
    fx_conc, fx_d1, fx_d2           the rows' shares x / (conc + d1 + d2) as floor(x * 2^32 / inf)

so sCF = 100 * fx_conc / (nq * 2^32) with a truncation below 2^-32 per row, and host adds, device adds and any order of
addition agree bit for bit.  Rows with a taxon >= T or a repeated taxon are counted in `skipped` only; a row induced
on no edge of the tree counts nowhere.

`sample_edge_quartets` draws the quartets around every branch on the caller's Generator; `run_scf` is the whole
computation on the resident matrix.
"""
from __future__ import annotations

import ctypes
from math import comb
from typing import Optional

import numpy as np

from ._handle import mask_bits
from .concordance import _TreeAccumulator, _div, newick_to_parent

WORDS = ("nq", "nq_zero", "sum_conc", "sum_d1", "sum_d2", "fx_conc", "fx_d1", "fx_d2")
FEATURES = ("sCF", "sDF1", "sDF2", "sN", "nq")
_FX = float(1 << 32)


class SiteConcordance(_TreeAccumulator):
    """Site concordance sums of class rows on one fixed tree.

    tree      newick text (tips = taxon numbers, or names through `samples`), or a parent array with `ntaxa`
    engine    a `QuartetEngine` for device adds (`add_dev`); None: host adds only
    """

    _prefix = "tq_scf"

    def __init__(self, tree, *, samples=None, ntaxa: int | None = None, engine=None):
        super().__init__(tree, samples, ntaxa, engine)

    # -- adding rows ------------------------------------------------------------------------------------------
    def add(self, sets, classes):
        """Host rows: sets u32[n,4] (any order of the four taxa) and their class rows u32[n,16]."""
        s = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1, 4)
        c = np.ascontiguousarray(classes, dtype=np.uint32).reshape(-1, 16)
        if c.shape[0] != s.shape[0]:
            raise ValueError("sets and classes must have the same number of rows")
        self._check(self._lib.tq_scf_add(self._h, s.ctypes.data, c.ctypes.data, s.shape[0]))

    def add_dev_ptrs(self, d_sets: int, d_classes: int, n: int, stream: int = 0):
        """Device rows by address (16-byte aligned), enqueued on `stream` (a hipStream_t as int)."""
        self._check(self._lib.tq_scf_add_dev(self._h, d_sets, d_classes, int(n), stream or None))

    def add_dev(self, sets, classes, stream=None):
        """Device rows as torch tensors on the engine's device: sets int32/uint32 [n,4], classes int32/uint32 [n,16];
        enqueued on `stream` (default: the current stream)."""
        self._need_engine()
        n = int(sets.numel()) // 4
        handle = self._dev_stream([(sets, 4, 4), (classes, 16, 4)], n, stream)
        self.add_dev_ptrs(sets.data_ptr(), classes.data_ptr(), n, handle)

    # -- reading -----------------------------------------------------------------------------------------------
    def raw(self) -> dict:
        """The summed words (waits for the device adds): edge_counts u64[E,8] in the order of `WORDS`, masks u64[E,W],
        skipped."""
        E, W = self.n_edges, self.mask_words
        counts = np.zeros((E, 8), np.int64)
        masks = np.zeros((E, W), np.uint64)
        skipped = ctypes.c_int64()
        self._check(self._lib.tq_scf_read(self._h, counts.ctypes.data, masks.ctypes.data, ctypes.byref(skipped)))
        return dict(edge_counts=counts.view(np.uint64), masks=masks, skipped=int(skipped.value))

    def split_masks(self) -> np.ndarray:
        """bool [E, T]: the taxa on one side of each edge (edge order and sides as `Concordance.split_masks`)."""
        m = np.zeros((self.n_edges, self.mask_words), np.uint64)
        self._check(self._lib.tq_scf_read(self._h, None, m.ctypes.data, None))
        return mask_bits(m, self.T)

    def stats(self) -> dict:
        """Per edge: split (bool [E,T]), nq, nq_zero, the six sums, sCF / sDF1 / sDF2 (means of the rows' shares, in
        percent), sN (mean decisive sites per row) and the pooled forms sCF_pooled / sDF1_pooled / sDF2_pooled
        (100 * sum_x / all decisive sites of the edge); NaN where the denominator is zero; and `skipped`."""
        r = self.raw()
        c = r["edge_counts"]
        out = {k: c[:, i].copy() for i, k in enumerate(WORDS)}
        out["split"] = mask_bits(r["masks"], self.T)
        nq = out["nq"].astype(np.float64)
        sums = [out[k].astype(np.float64) for k in ("sum_conc", "sum_d1", "sum_d2")]
        total = sums[0] + sums[1] + sums[2]
        for name, fx, s in zip(("sCF", "sDF1", "sDF2"), ("fx_conc", "fx_d1", "fx_d2"), sums):
            out[name] = 100.0 * _div(out[fx].astype(np.float64) / _FX, nq)
            out[name + "_pooled"] = 100.0 * _div(s, total)
        out["sN"] = _div(total, nq)
        out["skipped"] = r["skipped"]
        return out

    def to_newick(self) -> str:
        """The input tree (as given: rooted or not) with the statistics as comments, in the format of
        `Concordance.to_newick`: "[&sCF=..,sDF1=..,sDF2=..,sN=..,nq=..]" after the node of each edge (the first node,
        in preorder, whose clade is one side of the edge); tips carry their names."""
        st = self.stats()

        def feature(k, e):
            return f"{k}={int(st[k][e])}" if k == "nq" else f"{k}={'%.6g' % float(st[k][e])}"

        return self._annotated_newick(st["split"], lambda e: "[&" + ",".join(feature(k, e) for k in FEATURES) + "]",
                                      lambda t: "")


# -- the quartets around every branch -----------------------------------------------------------------------------
def _unrooted(parent, T):
    """Children lists of the tree with its unary nodes suppressed and a root of degree 2 dissolved, rooted at an
    internal node: (kids dict of internal node -> children, root)."""
    parent = np.asarray(parent, np.int64)
    n = len(parent)
    raw = [[] for _ in range(n)]
    root = -1
    for v, p in enumerate(parent):
        if p < 0:
            root = v
        else:
            raw[p].append(v)
    order = [root]
    for v in order:
        order.extend(raw[v])
    if len(order) != n:
        raise ValueError("the parent array is not one tree")
    rep, kids = {}, {}
    for v in reversed(order):
        if not raw[v]:
            if v >= T:
                raise ValueError("every tip must be a taxon")
            rep[v] = v
        elif len(raw[v]) == 1:
            rep[v] = rep[raw[v][0]]
        else:
            rep[v] = v
            kids[v] = [rep[k] for k in raw[v]]
    r = rep[root]
    if r not in kids:
        raise ValueError("the tree has fewer than 4 tips")
    if len(kids[r]) == 2:
        a, b = kids[r]
        if a not in kids:
            a, b = b, a
        if a not in kids:
            raise ValueError("the tree has fewer than 4 tips")
        kids[a].append(b)
        del kids[r]
        r = a
    return kids, r


def sample_edge_quartets(parent, ntaxa: int, per_edge: int, rng: np.random.Generator) -> np.ndarray:
    """For every nontrivial edge (u, v) of the tree `per_edge` draws: two different subtrees off u and two off v (on
    a binary tree the four subtrees around the branch), one taxon uniformly in each.  Host, NumPy, on the caller's
    Generator.  Returns the rows strictly ascending and unique, int64[n,4]."""
    T, per_edge = int(ntaxa), int(per_edge)
    kids, root = _unrooted(parent, T)
    # tips in preorder: the taxa of a subtree are contiguous in `tip_at`
    tip_at, lo, hi = [], {}, {}
    stack = [(root, False)]
    while stack:
        v, done = stack.pop()
        if done:
            hi[v] = len(tip_at)
        elif v in kids:
            lo[v] = len(tip_at)
            stack.append((v, True))
            stack.extend((k, False) for k in reversed(kids[v]))
        else:
            lo[v], hi[v] = len(tip_at), len(tip_at) + 1
            tip_at.append(v)
    if len(tip_at) != T or sorted(tip_at) != list(range(T)):
        raise ValueError(f"the tree's tips must be exactly the taxa 0..{T - 1}")
    tip_at = np.array(tip_at, np.int64)
    par = {k: u for u, ks in kids.items() for k in ks}

    def two_of(k):
        i = rng.integers(0, k, size=per_edge)
        j = rng.integers(0, k - 1, size=per_edge)
        return i, j + (j >= i)

    def taxon(parts, which):
        """parts i64[k,3] = (lo, hi, gap): the positions lo..hi-1 of `tip_at` without a gap of `gap` positions at lo."""
        p = parts[which]
        x = rng.integers(0, p[:, 1] - p[:, 0])
        return tip_at[np.where(p[:, 2] > 0, np.where(x < p[:, 0], x, x + p[:, 2]), p[:, 0] + x)]

    rows = []
    order = [root]
    for u in order:
        order.extend(k for k in kids[u] if k in kids)
    for v in order[1:]:
        u = par[v]
        below = np.array([(lo[k], hi[k], 0) for k in kids[v]], np.int64)
        above = [(lo[k], hi[k], 0) for k in kids[u] if k != v]
        if u != root:
            above.append((lo[u], T - (hi[u] - lo[u]) + lo[u], hi[u] - lo[u]))      # everything outside u's clade
        above = np.array(above, np.int64)
        i, j = two_of(len(below))
        k, m = two_of(len(above))
        rows.append(np.stack([taxon(below, i), taxon(below, j), taxon(above, k), taxon(above, m)], axis=1))
    if not rows or per_edge <= 0:
        return np.zeros((0, 4), np.int64)
    q = np.sort(np.concatenate(rows), axis=1)
    return np.unique(q, axis=0)


# -- the whole computation ----------------------------------------------------------------------------------------
def run_scf(engine, tmparr, tmpmap, tree, per_edge: Optional[int] = 100, subsample_snps: bool = False, seed=None,
            rng: Optional[np.random.Generator] = None, species_of=None, chunk: int = 1 << 20):
    """Site concordance factors of `tree` on the matrix (tmparr, tmpmap): `set_data`, then the quartets around every
    branch (`sample_edge_quartets` with `per_edge` draws on `rng`, or a Generator seeded with `seed`) or, with
    `per_edge=None`, all C(T,4) sets; per chunk of at most `chunk` rows the class rows (`patterns_dev`) and the add
    (`add_dev`) on the current stream; one read at the end.  `tree`: newick text whose tips are taxon numbers, or a
    parent array.  With `species_of` (i32[T], see `QuartetEngine.set_species`) the tree is a tree of species and the
    counts are those of the pooled lineages (full mode only).
    Returns (stats, newick, accumulator): `SiteConcordance.stats()`, `to_newick()` when the tree was given as text
    (else None) and the `SiteConcordance` itself."""
    import torch
    from ._lib import TetradHipError
    species = species_of is not None
    if species and subsample_snps:
        raise ValueError("species mode counts every site: subsample_snps must be False")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    rng = rng if rng is not None else np.random.default_rng(seed)
    engine.set_data(tmparr, tmpmap)
    if species:
        sp = np.asarray(species_of).reshape(-1)
        engine.set_species(sp)
        ntaxa = int(sp.max()) + 1
    else:
        ntaxa = engine.T
    acc = SiteConcordance(tree, ntaxa=ntaxa, engine=engine)
    if acc.T != ntaxa:
        acc.close()
        raise ValueError(f"the tree has {acc.T} taxa, the data {ntaxa}")
    sets = None if per_edge is None else sample_edge_quartets(acc.parent, ntaxa, per_edge, rng)
    total = comb(ntaxa, 4) if sets is None else len(sets)
    dev = torch.device("cuda", engine.device_id)
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev).cuda_stream
        d_classes = torch.empty((min(chunk, max(total, 1)), 16), dtype=torch.int32, device=dev)
        d_all = None if sets is None else torch.from_numpy(sets.astype(np.uint32).view(np.int32)).to(dev)
        for r0 in range(0, total, chunk):
            n = min(chunk, total - r0)
            if d_all is not None:
                d_sets = d_all[r0:r0 + n]
            elif species:                                    # the device unranks over the samples, not the species
                host = np.zeros((n, 4), np.uint32)
                rc = acc._lib.tq_unrank(None, r0, n, ntaxa, host.ctypes.data)
                if rc != 0:
                    raise TetradHipError(rc, "tq_unrank failed")
                d_sets = torch.from_numpy(host.view(np.int32)).to(dev)
            else:
                ranks = torch.arange(r0, r0 + n, dtype=torch.int64, device=dev)
                d_sets = torch.empty((n, 4), dtype=torch.int32, device=dev)
                engine.unrank_dev(ranks.data_ptr(), n, d_sets.data_ptr(), cur)
            if species:
                engine.patterns_species_dev(d_sets.data_ptr(), n, d_classes.data_ptr(), cur)
            else:
                engine.patterns_dev(d_sets.data_ptr(), n, subsample_snps, d_classes.data_ptr(), cur)
            acc.add_dev_ptrs(d_sets.data_ptr(), d_classes.data_ptr(), n, cur)
        stats = acc.stats()
    return stats, (acc.to_newick() if acc.newick is not None else None), acc
