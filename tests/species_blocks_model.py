"""Pure NumPy model of the pooled class rows of species sets per block of sites, two routes.

`literal_rows` is the definition: the sum, over every lineage quartet (i in A, j in B, k in C, l in D) taken in that
role order, of the block rows `blocks_model.block_rows` counts for it from the raw columns (full mode, invariant sites
not counted).  `factored_rows` is the form the pooled matrix of section 12 has: per-species base counts
(`species_model.species_counts`), the products a[x] b[y] c[z] d[w] summed over the sites of a block, reduced to classes
by the equality rule of `patterns_model`, class 0 zeroed.  Neither knows about partitions or their inversion.
"""
from __future__ import annotations

from itertools import product

import numpy as np

import blocks_model as bm
import patterns_model as pm
from species_model import members, species_counts


def pattern_classes() -> np.ndarray:
    """i64[256]: the class of pattern 64 x0 + 16 x1 + 4 x2 + x3, by `patterns_model.site_classes`."""
    grid = np.array(list(product(range(4), repeat=4)), np.uint8).T            # [4, 256], column p = pattern p
    return pm.site_classes(grid)


def rows_of_bins(bins) -> np.ndarray:
    """[..., 256] pattern counts (Python-int safe i64) -> [..., 16] class rows: class 0 zeroed, slot 15 = the sum of
    slots 1..14."""
    bins = np.asarray(bins, np.int64)
    cls = pattern_classes()
    out = np.zeros(bins.shape[:-1] + (16,), np.int64)
    for k in range(1, 15):
        out[..., k] = bins[..., cls == k].sum(axis=-1)
    out[..., 15] = out[..., 1:15].sum(axis=-1)
    return out


def site_bins(cnt, sset) -> np.ndarray:
    """i64[S,256]: a[x] b[y] c[z] d[w] at every site for the species set (A, B, C, D) of the count table i64[K,S,4]."""
    a, b, c, d = (np.asarray(cnt[int(k)], np.int64) for k in sset)
    t = a[:, :, None, None, None] * b[:, None, :, None, None] * c[:, None, None, :, None] * d[:, None, None, None, :]
    return t.reshape(a.shape[0], 256)


def factored_rows(cnt, ssets, block_starts) -> np.ndarray:
    """u32[Q,B,16] from the count table i64[K,S,4] (`species_counts`, or haplotype counts in allele mode): the bins of
    every block = the products summed over its slice of sites, then the class rule."""
    ssets = np.asarray(ssets).reshape(-1, 4)
    starts = [int(v) for v in np.asarray(block_starts).reshape(-1)]
    B = len(starts) - 1
    out = np.zeros((ssets.shape[0], B, 16), np.int64)
    for r, sset in enumerate(ssets):
        # sums over slices as differences of running sums (exact in i64: a bin's total is below 2^32 x S)
        run = np.concatenate([np.zeros((1, 256), np.int64), np.cumsum(site_bins(cnt, sset), axis=0)])
        bins = np.stack([run[starts[j + 1]] - run[starts[j]] for j in range(B)])
        out[r] = rows_of_bins(bins)
    assert out.min(initial=0) >= 0 and out.max(initial=0) < 2**32
    return out.astype(np.uint32)


def factored_rows_of(tmparr, species_of, K, ssets, block_starts) -> np.ndarray:
    return factored_rows(species_counts(np.asarray(tmparr), species_of, K), ssets, block_starts)


def literal_rows(tmparr, species_of, K, ssets, block_starts) -> np.ndarray:
    """u32[Q,B,16]: the sum of `blocks_model.block_rows` over the lineage quartets of every species set (small cases)."""
    mem = members(species_of, K)
    ssets = np.asarray(ssets).reshape(-1, 4)
    B = len(np.asarray(block_starts).reshape(-1)) - 1
    out = np.zeros((ssets.shape[0], B, 16), np.int64)
    for r, sset in enumerate(ssets):
        lin = np.array(list(product(*(mem[int(k)] for k in sset))), np.int64).reshape(-1, 4)
        if lin.shape[0]:
            out[r] = bm.block_rows(tmparr, lin, block_starts, count_invariant=False).sum(axis=0, dtype=np.int64)
    assert out.max(initial=0) < 2**32
    return out.astype(np.uint32)


def pack_counts(counts) -> np.ndarray:
    """[..., 4] counts {n_A, n_C, n_G, n_T} <= 255 -> the packed u32 word of the species table."""
    c = np.asarray(counts, np.int64)
    assert c.min(initial=0) >= 0 and c.max(initial=0) <= 255
    return (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | (c[..., 3] << 24)).astype(np.uint32)


def site_row(counts4) -> np.ndarray:
    """One site: counts [4 species, 4 bases] -> the class row i64[16] by enumeration of the 256 patterns."""
    return rows_of_bins(site_bins(np.asarray(counts4, np.int64)[:, None, :], (0, 1, 2, 3))[0])
