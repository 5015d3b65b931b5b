"""Pure-Python model of species-mode pooling, pinned to the oracle's count function.

`pooled_literal` is the definition: the sum, over every lineage quartet of a species quartet, of the full-mode
count matrices the reference worker builds (oracle.full_chunk_to_matrices, which restates resolve_quartets.py:76-104,
under the worker's mask of :216-223).  `pooled_factored` is the form the kernel computes: per-species base counts,
one outer product per site, the invariant bins zeroed.
"""
from __future__ import annotations

from itertools import product

import numpy as np


def flattenings(t4: np.ndarray) -> np.ndarray:
    """u32[..., 4,4,4,4] tensor T[x,y,z,w] -> u32[..., 3,16,16]: rows (x,y) | (x,z) | (x,w), the layout of cmats."""
    lead = t4.shape[:-4]
    m0 = t4.reshape(*lead, 16, 16)
    m1 = np.swapaxes(t4, -3, -2).reshape(*lead, 16, 16)
    m2 = np.moveaxis(t4, -1, -3).reshape(*lead, 16, 16)
    return np.stack([m0, m1, m2], axis=-3)


def worker_mask(seqs: np.ndarray) -> np.ndarray:
    """resolve_quartets.py:216-223: a base missing (> 3) or all four bases equal."""
    return (seqs > 3).any(axis=0) | (seqs == seqs[0]).all(axis=0)


def members(species_of, K):
    species_of = np.asarray(species_of)
    return [np.flatnonzero(species_of == k) for k in range(K)]


def pooled_literal(orc, tmparr, tmpmap, species_of, K, squartets) -> np.ndarray:
    """u32[Q,3,16,16]: sum over lineage quartets of oracle.full_chunk_to_matrices (small cases only)."""
    mem = members(species_of, K)
    locus = np.asarray(tmpmap)[:, 0]
    out = np.zeros((len(squartets), 3, 16, 16), np.uint64)
    for r, sq in enumerate(np.asarray(squartets)):
        for lin in product(*(mem[k] for k in sq)):
            seqs = tmparr[list(lin)]
            out[r] += orc.full_chunk_to_matrices(seqs, locus, worker_mask(seqs))
    return out.astype(np.uint32)


def species_counts(tmparr, species_of, K) -> np.ndarray:
    """i64[K,S,4]: lineages of each species with base x at each site (missing cells count nowhere)."""
    T, S = tmparr.shape
    cnt = np.zeros((K, S, 4), np.int64)
    for t in range(T):
        k = int(species_of[t])
        if k < 0:
            continue
        row = tmparr[t]
        ok = row <= 3
        cnt[k, np.flatnonzero(ok), row[ok]] += 1
    return cnt


def pooled_factored(tmparr, species_of, K, squartets, counts=None) -> np.ndarray:
    """u32[Q,3,16,16]: sum_s a_s (x) b_s (x) c_s (x) d_s with the bins (x,x,x,x) zeroed."""
    cnt = species_counts(tmparr, species_of, K) if counts is None else counts
    sq = np.asarray(squartets)
    out = np.zeros((len(sq), 4, 4, 4, 4), np.int64)
    S = cnt.shape[1]
    per_site = cnt.sum(axis=2)                      # lineages with a base, per species and site
    for r, (a, b, c, d) in enumerate(sq):
        # every bin, and every partial sum of it, is a non-negative integer <= this total: below 2^53 the float64
        # product (AB)^T (CD) of the two S x 16 outer-product panels is exact in any summation order (and runs in BLAS;
        # the int64 einsum takes seconds per row at a million sites)
        if int((per_site[a] * per_site[b] * per_site[c] * per_site[d]).sum()) < 2**53:
            ab = (cnt[a][:, :, None] * cnt[b][:, None, :]).reshape(S, 16).astype(np.float64)
            cd = (cnt[c][:, :, None] * cnt[d][:, None, :]).reshape(S, 16).astype(np.float64)
            t = (ab.T @ cd).astype(np.int64).reshape(4, 4, 4, 4)
        else:
            t = np.einsum("sx,sy,sz,sw->xyzw", cnt[a], cnt[b], cnt[c], cnt[d], optimize=True)
        for x in range(4):
            t[x, x, x, x] = 0
        out[r] = t
    assert out.max(initial=0) < 2**32
    return flattenings(out.astype(np.uint32))


def score_rows(orc, cmats):
    """(rstat u32[Q,2], rscor f64[Q,3], zero-data bool[Q]) of pooled matrices through oracle.score_from_cmats."""
    Q = cmats.shape[0]
    rstat = np.zeros((Q, 2), np.uint32)
    rscor = np.full((Q, 3), 0.001)
    zero = np.zeros(Q, bool)
    for q in range(Q):
        n = int(cmats[q, 0].sum(dtype=np.uint64))
        rstat[q, 1] = n
        if n == 0:
            zero[q] = True
            continue
        _, _, scor, topo = orc.score_from_cmats(cmats[q])
        rscor[q] = scor
        rstat[q, 0] = topo
    return rstat, rscor, zero


def check_rows(rstat, rscor, flags, cm, orc):
    """Rows against the pooled matrices `cm` scored by the oracle: nsnps exact, the zero-data flag, topology on
    unflagged rows, scores within the bar of __graft_entry__.smoke."""
    m_rstat, m_rscor, zero = score_rows(orc, cm)
    assert np.array_equal(rstat[:, 1], m_rstat[:, 1])
    assert np.array_equal((flags & 1) != 0, zero)
    ok = (flags & 3) == 0
    assert np.array_equal(rstat[ok, 0], m_rstat[ok, 0])
    smax = np.array([np.linalg.svd(c.astype(np.float64), compute_uv=False).max() if c.any() else 0.0 for c in cm[:, 0]])
    live = ~zero
    assert np.all(np.abs(rscor[live] - m_rscor[live]) <= 1e-6 * np.abs(m_rscor[live]) + 1e-12 * smax[live, None])


def lineage_data(sizes, S, seed, missing=0.0, p_within=0.0, left_out=1):
    """(tmparr u8[T,S], tmpmap, species_of i32[T]) for species of the given sizes: one sequence per species from
    `synth.simulate_species(K, 1, S)` (sites evolved down a random species tree), copied to each of its lineages with
    a `p_within` share of cells redrawn and a `missing` share set to N; samples in random order, `left_out` of them
    in no species.  With both shares 0 a species of n lineages has a count of n at every site."""
    from tetrad_amd import synth
    K = len(sizes)
    rng = np.random.default_rng([seed, S, K])
    base, tmpmap, order, _ = synth.simulate_species(K, 1, S, seed, p_within=0.0, missing=0.0)
    seq = np.empty_like(base)
    seq[order] = base                                   # row k = the sequence of species k
    sp = rng.permutation(np.concatenate([np.repeat(np.arange(K), sizes), np.full(left_out, -1)])).astype(np.int32)
    tmparr = seq[np.maximum(sp, 0)]
    mut = rng.random(tmparr.shape) < p_within
    tmparr[mut] = rng.integers(0, 4, size=int(mut.sum()), dtype=np.uint8)
    tmparr[rng.random(tmparr.shape) < missing] = 78
    return np.ascontiguousarray(tmparr), tmpmap, sp


def spike_data(S, n=11):
    """Four species of `n` lineages, each the copies of one sequence; 60 % of the sites hold the pattern (0, 0, 1, 1)
    across the four species, the rest is uniform.  At n = 11 and S = 293 000 the pooled row (0, 1, 2, 3) has a bin of
    2 579 729 559 >= 2^31 and nsnps = 4 263 722 738."""
    rng = np.random.default_rng(0)
    base = rng.integers(0, 4, size=(4, S)).astype(np.uint8)
    spike = rng.random(S) < 0.6
    base[:, spike] = np.array([0, 0, 1, 1], np.uint8)[:, None]
    return np.repeat(base, n, axis=0), np.repeat(np.arange(4, dtype=np.int32), n)


def parse_tips_newick(text: str):
    """Bipartitions (frozensets of tip ids, the side without the smallest tip) of a numeric-tip newick."""
    text = text.strip().rstrip(";")
    pos = 0

    def node():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            kids = [node()]
            while text[pos] == ",":
                pos += 1
                kids.append(node())
            assert text[pos] == ")"
            pos += 1
            while pos < len(text) and text[pos] not in ",)":
                pos += 1              # internal labels / lengths
            return frozenset().union(*(k[0] for k in kids)), kids
        j = pos
        while pos < len(text) and text[pos] not in ",)":
            pos += 1
        return frozenset([int(text[j:pos].split(":")[0])]), None

    root, _ = node()
    clades = []

    def walk(t):
        s, kids = t
        clades.append(s)
        for k in kids or ():
            walk(k)

    pos = 0
    walk(node())
    allt = root
    lo = min(allt)
    splits = set()
    for c in clades:
        side = c if lo not in c else allt - c
        if 2 <= len(side) <= len(allt) - 2:
            splits.add(frozenset(side))
    return splits, allt


def quartet_topology(splits, q) -> int | None:
    """0 / 1 / 2 for ab|cd, ac|bd, ad|bc under the tree's splits; None if unresolved."""
    a, b, c, d = (int(x) for x in q)
    for t, (p1, p2) in enumerate((((a, b), (c, d)), ((a, c), (b, d)), ((a, d), (b, c)))):
        for s in splits:
            if (p1[0] in s) == (p1[1] in s) and (p2[0] in s) == (p2[1] in s) and (p1[0] in s) != (p2[0] in s):
                return t
    return None
