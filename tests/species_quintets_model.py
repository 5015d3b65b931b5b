"""Pure NumPy model of the pooled five-taxon class rows of species sets per block of sites, two
routes that know nothing of multi-dots.

`literal_rows` is the definition: the sum, over every lineage quintet (one lineage per species, in position order), of the
block rows `quintets_model.block_rows` counts for it from the raw columns.  `factored_rows` is the form the pooled counts
have: per-species base counts (`species_model.species_counts`), the products n0[x0] n1[x1] n2[x2] n3[x3] n4[x4] of all
1024 patterns summed over the sites of a block, reduced to classes by `quintets_model.class_table`.
"""
from __future__ import annotations

from itertools import product

import numpy as np

import quintets_model as qm
from species_model import members, species_counts


def rows_of_bins(bins) -> np.ndarray:
    """[..., 1024] pattern counts (i64) -> [..., 16] class rows: slot k = 1..15 the patterns of class k, slot 0 their sum;
    patterns of class 0 (invariant, three or four bases) count nowhere."""
    bins = np.asarray(bins, np.int64)
    cls = qm.class_table()
    out = np.zeros(bins.shape[:-1] + (16,), np.int64)
    for k in range(1, 16):
        out[..., k] = bins[..., cls == k].sum(axis=-1)
    out[..., 0] = out[..., 1:].sum(axis=-1)
    return out


def site_bins(cnt, sset5) -> np.ndarray:
    """i64[S,1024]: n0[x0] n1[x1] n2[x2] n3[x3] n4[x4] at every site for the species set of the count table i64[K,S,4];
    index 256 x0 + 64 x1 + 16 x2 + 4 x3 + x4."""
    a, b, c, d, e = (np.asarray(cnt[int(k)], np.int64) for k in sset5)
    t = (a[:, :, None, None, None, None] * b[:, None, :, None, None, None] * c[:, None, None, :, None, None] *
         d[:, None, None, None, :, None] * e[:, None, None, None, None, :])
    return t.reshape(a.shape[0], 1024)


def running_rows(cnt, sset5) -> np.ndarray:
    """i64[S + 1,16]: the class rows of the sites of one species set (the class table applied to the 1024 products of
    every site), summed over the sites before s (exact in i64: a slot's total is below 2^32 x S)."""
    return np.concatenate([np.zeros((1, 16), np.int64), np.cumsum(rows_of_bins(site_bins(cnt, sset5)), axis=0)])


def factored_rows(cnt, ssets5, block_starts, running=running_rows) -> np.ndarray:
    """u32[Q,B,16] from the count table i64[K,S,4] (`species_counts`, or haplotype counts in allele mode): a block's row
    is the sum of its sites' class rows, taken as a difference of running sums.  `running` lets a caller that asks for
    many block shapes of the same sets keep the running sums."""
    ssets5 = np.asarray(ssets5).reshape(-1, 5)
    starts = [int(v) for v in np.asarray(block_starts).reshape(-1)]
    B = len(starts) - 1
    out = np.zeros((ssets5.shape[0], B, 16), np.int64)
    for r, sset in enumerate(ssets5):
        run = running(cnt, sset)
        out[r] = np.stack([run[starts[j + 1]] - run[starts[j]] for j in range(B)])
    assert out.min(initial=0) >= 0 and out.max(initial=0) < 2**32
    return out.astype(np.uint32)


def factored_rows_of(tmparr, species_of, K, ssets5, block_starts) -> np.ndarray:
    return factored_rows(species_counts(np.asarray(tmparr), species_of, K), ssets5, block_starts)


def literal_rows(tmparr, species_of, K, ssets5, block_starts) -> np.ndarray:
    """u32[Q,B,16]: the sum of `quintets_model.block_rows` over the lineage quintets of every species set (small cases)."""
    mem = members(species_of, K)
    ssets5 = np.asarray(ssets5).reshape(-1, 5)
    B = len(np.asarray(block_starts).reshape(-1)) - 1
    out = np.zeros((ssets5.shape[0], B, 16), np.int64)
    for r, sset in enumerate(ssets5):
        lin = np.array(list(product(*(mem[int(k)] for k in sset))), np.int64).reshape(-1, 5)
        if lin.shape[0]:
            out[r] = qm.block_rows(tmparr, lin, block_starts).sum(axis=0, dtype=np.int64)
    assert out.max(initial=0) < 2**32
    return out.astype(np.uint32)


def site_row(counts5) -> np.ndarray:
    """One site: counts [5 species, 4 bases] -> the class row i64[16] by enumeration of the 1024 patterns (Python ints
    through object arithmetic are not needed: 255^5 x 1024 < 2^63)."""
    return rows_of_bins(site_bins(np.asarray(counts5, np.int64)[:, None, :], (0, 1, 2, 3, 4))[0])
