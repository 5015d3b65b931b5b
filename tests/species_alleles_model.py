"""Pure-NumPy model of species mode read from both alleles of IUPAC genotypes.

Every sample of the source matrix is two haplotype lineages; the pooled matrix of a species quartet is the pooled matrix
of `species_model` over those haplotypes.  Nothing here draws a coin.
"""
from __future__ import annotations

import numpy as np

from species_model import pooled_factored

#: source byte -> its two alleles as 0..3 (A C G T): the two-base codes are the table of bootstrap.hpp::tq_boot_build_kernel
ALLELES = {65: (0, 0), 67: (1, 1), 71: (2, 2), 84: (3, 3), 0: (0, 0), 1: (1, 1), 2: (2, 2), 3: (3, 3),
           82: (2, 0), 75: (2, 3), 83: (2, 1), 89: (3, 1), 87: (3, 0), 77: (1, 0)}      # R K S Y W M


def haplotypes(seqarr) -> np.ndarray:
    """u8[2T,S]: rows 2t and 2t+1 are the two alleles of sample t as 0..3, or 78 for every byte that is no base and no
    two-base code (N, gap, three-base codes, anything else)."""
    seqarr = np.asarray(seqarr, dtype=np.uint8)
    lut = np.full((256, 2), 78, np.uint8)
    for v, pair in ALLELES.items():
        lut[v] = pair
    T, S = seqarr.shape
    return np.ascontiguousarray(lut[seqarr].transpose(0, 2, 1).reshape(2 * T, S))


def replicate_columns(spans, lidxs) -> np.ndarray:
    """i64[S]: the source columns of the drawn loci, concatenated in draw order and unshuffled inside each locus."""
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    parts = [np.arange(spans[l, 0], spans[l, 1]) for l in np.asarray(lidxs, dtype=np.int64)]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def pooled_alleles(seqarr, species_of, K, squartets, cols=None) -> np.ndarray:
    """u32[Q,3,16,16]: pooled count matrices of species quartets over the haplotype lineages of the source columns
    `cols` (all columns when None)."""
    hap = haplotypes(seqarr)
    if cols is not None:
        hap = np.ascontiguousarray(hap[:, np.asarray(cols, dtype=np.int64)])
    return pooled_factored(hap, np.repeat(np.asarray(species_of), 2), K, squartets)


# -- the bootstrap loop's test case, shared by the CPU check of its parameters and the GPU test of the loop ---------------
LOOP_K, LOOP_N, LOOP_S0, LOOP_NBOOTS, LOOP_SEED = 8, 3, 6000, 6, 17


def loop_source():
    """(seqarr u8[24,6000] with 15 % two-base codes and 10 % missing, spans, species_of, generating species tree)."""
    from tetrad_amd import synth
    tmparr, tmpmap, species_of, nwk = synth.simulate_species(LOOP_K, LOOP_N, LOOP_S0, seed=23)
    seqarr, _, spans = synth.make_c5_source(source=(tmparr, tmpmap), ambiguous=0.15)
    return seqarr, spans, species_of, nwk


def loop_draws(nloci, nquartets, K=LOOP_K, nboots=LOOP_NBOOTS, seed=LOOP_SEED):
    """The draws `species.bootstrap_species_trees` makes on one Generator, replicate by replicate:
    [(lidxs, seed_shuffle, seed_ambig, squartets)]."""
    from math import comb
    from tetrad_amd import species
    from tetrad_amd.bootstrap import draw_replicate
    rng = np.random.default_rng(seed)
    sampled = 0 < nquartets < comb(K, 4)
    out = []
    for _ in range(nboots):
        lidxs, s1, s2 = draw_replicate(nloci, rng)
        sq = species.species_quartets(K, nquartets, int(rng.integers(2**31))) if sampled else species.species_quartets(K)
        out.append((lidxs, s1, s2, sq))
    return out
