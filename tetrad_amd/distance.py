"""Pairwise taxon distances from the SNP matrix and neighbour-joining trees on them.

How far apart are two samples, and how much data do they share?  For every pair of taxa and every block of sites the
library counts, exactly and as integers (`tq_taxon_counts*`, tetrad_amd/csrc/taxdist.hpp), the sites both hold, the
sites where they differ, and of those the transitions and transversions -- on the resident replicate of a
`QuartetEngine` (`engine.taxon_counts`, a HIP kernel on the bit planes) or on the host from the u8 matrix
(`taxon_counts_host`).  Both give identical arrays.  Everything else here is derived from those counts: distances under
three models, the shared-site matrix, pooled counts between populations, neighbour-joining trees (`tq_nj_tree`, host code)
and their jackknife or bootstrap supports through `consensus.Consensus`.  No reference counterpart.

Definitions.  A pair row is (both, diff, ts, tv): the sites present (`tmparr <= 3`) in both taxa,
of those the sites whose bases differ, of those the transitions (A<->G, C<->T), and tv = diff - ts.  Row (i, i) is
(sites present in i, 0, 0, 0).  Full mode: every site counts.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import TetradHipError

MODELS = ("p", "jc", "kimura")


def _check(rc: int, what: str):
    if rc != 0:
        raise TetradHipError(rc, (_lib.load().tq_last_error(None) or b"").decode() or f"{what} failed")


def block_starts_of(block_starts, S: int) -> np.ndarray:
    """`block_starts` as i64[B + 1]; None means one block [0, S)."""
    if block_starts is None:
        return np.array([0, int(S)], np.int64)
    b = np.ascontiguousarray(block_starts, dtype=np.int64).reshape(-1)
    if b.shape[0] < 2:
        raise ValueError("block_starts must hold B + 1 >= 2 boundaries")
    return b


def taxon_counts_host(tmparr, block_starts=None) -> np.ndarray:
    """Pair rows u32[B, T, T, 4] of `tmparr` u8[T, S] per block of sites, on the host (no GPU, no engine)."""
    arr = np.ascontiguousarray(tmparr, dtype=np.uint8)
    if arr.ndim != 2:
        raise ValueError("tmparr must be 2-D [ntaxa, nsites]")
    T, S = arr.shape
    b = block_starts_of(block_starts, S)
    B = b.shape[0] - 1
    out = np.zeros((B, T, T, 4), np.uint32)
    _check(_lib.load().tq_taxon_counts_host(arr.ctypes.data, T, S, b.ctypes.data, B, out.ctypes.data), "tq_taxon_counts_host")
    return out


# -- derived quantities ---------------------------------------------------------------------------------------------
def distances(counts, model: str = "jc") -> np.ndarray:
    """f64[..., T, T] from counts [..., T, T, 4] (u32 rows or int64 sums): "p" = diff / both; "jc" = -0.75 ln(1 - 4p/3)
    (Jukes & Cantor 1969); "kimura" = -0.5 ln((1 - 2P - Q) sqrt(1 - 2Q)) with P = ts / both, Q = tv / both (Kimura 1980).
    NaN where both = 0, +inf where a logarithm's argument is not positive, 0 on the diagonal."""
    if model not in MODELS:
        raise ValueError(f"no distance model {model!r}: one of {MODELS}")
    c = np.asarray(counts)
    if c.ndim < 3 or c.shape[-1] != 4 or c.shape[-2] != c.shape[-3]:
        raise ValueError("counts must be [..., T, T, 4]")
    c = c.astype(np.float64)
    both = c[..., 0]
    have = both > 0
    safe = np.where(have, both, 1.0)

    def neg_log(arg, scale):
        ok = arg > 0
        return np.where(ok, -scale * np.log(np.where(ok, arg, 1.0)), np.inf)

    if model == "p":
        d = c[..., 1] / safe
    elif model == "jc":
        d = neg_log(1.0 - 4.0 * (c[..., 1] / safe) / 3.0, 0.75)
    else:
        P, Q = c[..., 2] / safe, c[..., 3] / safe
        a, b = 1.0 - 2.0 * P - Q, 1.0 - 2.0 * Q
        ok = (a > 0) & (b > 0)
        d = np.where(ok, -0.5 * np.log(np.where(ok, a * np.sqrt(np.where(ok, b, 1.0)), 1.0)), np.inf)
    d = np.where(have, d, np.nan) + 0.0                        # + 0.0: no negative zero
    T = d.shape[-1]
    d[..., np.arange(T), np.arange(T)] = 0.0
    return d


def sharing(counts):
    """(both int64[..., T, T], Jaccard f64[..., T, T]): the sites two taxa share, and both / (n_i + n_j - both) with n
    the sites present in a taxon (the diagonal); 0.0 where the denominator is 0."""
    both = np.asarray(counts)[..., 0].astype(np.int64)
    n = np.diagonal(both, axis1=-2, axis2=-1)
    den = n[..., :, None] + n[..., None, :] - both
    jac = np.zeros(both.shape, np.float64)
    np.divide(both, den, out=jac, where=den != 0)
    return both, jac


def fill_undefined(dist, factor: float = 2.0) -> np.ndarray:
    """A copy of `dist` whose non-finite off-diagonal entries are `factor` times the largest finite off-diagonal one: an
    explicit choice of the caller for pairs without shared sites or past a model's range; nothing does it silently."""
    d = np.array(dist, dtype=np.float64)
    T = d.shape[-1]
    off = ~np.eye(T, dtype=bool)
    finite = np.isfinite(d) & off
    if not finite.any():
        raise ValueError("no finite off-diagonal distance to scale")
    d[~np.isfinite(d) & off] = float(factor) * d[finite].max()
    return d


def pool_counts(counts, species_of, K: int | None = None) -> np.ndarray:
    """int64[..., K, K, 4] from counts [..., T, T, 4] and `species_of` [T] (species id per taxon, -1 = left out): entry
    (A, B), A != B, is the sum over the lineages a in A and b in B; entry (A, A) the sum over the unordered pairs inside A
    (zeros for a single member).  `distances` on it gives the mean between- and within-population distances."""
    c = np.asarray(counts).astype(np.int64)
    sp = np.asarray(species_of, dtype=np.int64).reshape(-1)
    T = c.shape[-2]
    if c.shape[-1] != 4 or c.shape[-3] != T or sp.shape[0] != T:
        raise ValueError("counts must be [..., T, T, 4] and species_of [T]")
    if K is None:
        K = int(sp.max()) + 1 if T else 0
    if (sp >= K).any():
        raise ValueError("a species id is not below K")
    M = np.zeros((T, int(K)), np.int64)
    M[np.flatnonzero(sp >= 0), sp[sp >= 0]] = 1
    full = np.einsum("ta,...tuc,ub->...abc", M, c, M)          # ordered pairs, the diagonal rows included
    diag = np.einsum("ta,...tc->...ac", M, c[..., np.arange(T), np.arange(T), :])
    idx = np.arange(int(K))
    full[..., idx, idx, :] = (full[..., idx, idx, :] - diag) // 2
    return full


# -- trees ---------------------------------------------------------------------------------------------------------
def nj(dist):
    """Neighbour joining (`tq_nj_tree`): (parent i32[2T - 2], length f64[2T - 2]) of `dist` f64[T, T], T >= 3; tips are
    0..T-1, parent[root] = -1.  A non-finite or asymmetric off-diagonal entry is refused (see `fill_undefined`)."""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("dist must be [T, T]")
    T = d.shape[0]
    n = max(2 * T - 2, 1)
    parent = np.full(n, -1, np.int32)
    length = np.zeros(n, np.float64)
    _check(_lib.load().tq_nj_tree(d.ctypes.data, T, parent.ctypes.data, length.ctypes.data), "tq_nj_tree")
    return parent, length


def nj_parents(dist) -> np.ndarray:
    """The parent array of the neighbour-joining tree alone."""
    return nj(dist)[0]


def parent_to_newick(parent, length=None, samples=None, labels=None) -> str:
    """Newick text of a parent array (tips 0..T-1, parent[root] = -1), children in ascending node id; `length` adds
    branch lengths (repr of the float, so the text reads back exactly), `labels` {node: text} labels internal nodes."""
    par = np.asarray(parent, dtype=np.int64).reshape(-1)
    n = par.shape[0]
    kids = [[] for _ in range(n)]
    root = -1
    for v in range(n):
        if par[v] < 0:
            root = v
        else:
            kids[par[v]].append(v)
    names = None if samples is None else (dict(samples) if hasattr(samples, "items") else dict(enumerate(samples)))
    out, stack = [], [(root, 0)]
    while stack:
        v, i = stack.pop()
        if i == 0 and kids[v]:
            out.append("(")
        if i < len(kids[v]):
            if i:
                out.append(",")
            stack.append((v, i + 1))
            stack.append((kids[v][i], 0))
            continue
        if kids[v]:
            out.append(")")
            if labels and v in labels:
                out.append(str(labels[v]))
        else:
            out.append(str(v) if names is None else str(names[v]))
        if length is not None and v != root:
            out.append(":" + repr(float(length[v])))
    return "".join(out) + ";"


def nj_tree(dist, samples=None):
    """(newick with branch lengths, parent, length) of the neighbour-joining tree of `dist`."""
    parent, length = nj(dist)
    return parent_to_newick(parent, length, samples), parent, length


def jackknife_nj_trees(block_counts, model: str = "jc") -> list:
    """The B parent arrays of the delete-one-block trees of `block_counts` [B, T, T, 4]: tree j is neighbour joining on
    `distances` of the total minus block j (int64)."""
    c = np.asarray(block_counts).astype(np.int64)
    total = c.sum(axis=0)
    return [nj_parents(distances(total - c[j], model)) for j in range(c.shape[0])]


def bootstrap_nj_trees(engine, seqarr, spans, nboots: int, rng, model: str = "jc", consensus=None) -> list:
    """The parent arrays of `nboots` bootstrap replicate trees: `set_source` once, then per replicate
    `resample_tmp_database` (the replicate is built on the device), `taxon_counts()` and neighbour joining.  With
    `consensus` (a `consensus.Consensus`) the trees are added to it as well."""
    from .bootstrap import resample_tmp_database
    rng = np.random.default_rng(rng)
    engine.set_source(seqarr, spans)
    parents = []
    for _ in range(int(nboots)):
        resample_tmp_database(engine, rng)
        parents.append(nj_parents(distances(engine.taxon_counts()[0], model)))
    if consensus is not None and parents:
        consensus.add_parents(parents)
    return parents


def clade_masks(parent, T: int) -> dict:
    """{node: bool[T]} the taxa below every internal node but the root."""
    par = np.asarray(parent, dtype=np.int64).reshape(-1)
    below = np.zeros((par.shape[0], T), bool)
    below[np.arange(T), np.arange(T)] = True
    depth = np.zeros(par.shape[0], np.int64)
    for v in range(par.shape[0]):
        u, k = v, 0
        while par[u] >= 0:
            u, k = par[u], k + 1
        depth[v] = k
    for v in np.argsort(-depth, kind="stable"):
        if par[v] >= 0:
            below[par[v]] |= below[v]
    return {v: below[v] for v in range(T, par.shape[0]) if par[v] >= 0}


def run_distance_tree(engine, tmparr, tmpmap, model: str = "jc", nblocks: int = 50, samples=None):
    """(newick, counts): the neighbour-joining tree of the whole matrix with branch lengths and, on every internal
    branch, the integer percent of the delete-one-block jackknife trees that hold it (`Consensus` over the blocks of
    `patterns.locus_blocks`); counts are the block rows u32[B, T, T, 4]."""
    from .consensus import Consensus, percent
    from .patterns import locus_blocks
    engine.set_data(tmparr, tmpmap)
    counts = engine.taxon_counts(locus_blocks(tmpmap, nblocks))
    T = counts.shape[1]
    parent, length = nj(distances(counts.astype(np.int64).sum(axis=0), model))
    trees = jackknife_nj_trees(counts, model)
    labels = {}
    with Consensus(T, engine=engine) as cons:
        cons.add_parents(trees)
        got, masks = cons.support_of(parent)
        seen = {}
        for c, m in zip(got, masks):
            seen[m.tobytes()] = seen[(~m).tobytes()] = percent(int(c), len(trees))
        for v, m in clade_masks(parent, T).items():
            if m.tobytes() in seen:
                labels[v] = seen[m.tobytes()]
    return parent_to_newick(parent, length, samples, labels), counts
