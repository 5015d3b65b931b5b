"""Species mode from both alleles on the CPU: the haplotype model against the expectation of the
coin-resolved lineage-quartet sum, its no-ambiguity case, the range rule in lineages and the replicate column helper."""
from itertools import combinations, product

import numpy as np
import pytest

from species_alleles_model import ALLELES, haplotypes, pooled_alleles, replicate_columns
from species_model import pooled_factored, pooled_literal
from tetrad_amd import species, synth

ASCII = np.array([65, 67, 71, 84], np.uint8)
# (sample, site, code): six heterozygous cells, every two-base code once; two share a site, two share a sample
HET_CELLS = [(0, 3, 82), (1, 3, 75), (1, 17, 83), (2, 8, 89), (3, 30, 87), (4, 39, 77)]


def het_case():
    rng = np.random.default_rng(40)
    seqarr = ASCII[rng.integers(0, 4, size=(5, 40))]
    seqarr[rng.random(seqarr.shape) < 0.1] = 78
    seqarr[2, 5], seqarr[0, 9] = 45, 66                 # a gap and a three-base code: missing
    for t, s, code in HET_CELLS:
        seqarr[t, s] = code
    return seqarr


@pytest.mark.parametrize("species_of", [(0, 0, 1, 2, 3), (3, 1, 1, 0, 2), (0, 1, 2, 3, 4)])
def test_alleles_equal_16_times_the_coin_expectation(oracle, species_of):
    """16 x the mean over all 2^6 coin resolutions of the literal lineage-quartet sum (the reference's count function on
    every resolved matrix) equals the haplotype model exactly.  Rows of four different species: a row that repeats a
    species pairs a sample with itself, which has no lineage-quartet counterpart with independent alleles."""
    seqarr = het_case()
    sp = np.array(species_of, np.int32)
    K = int(sp.max()) + 1
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    tmpmap = np.stack([np.arange(40) // 4, np.arange(40)], axis=1).astype(np.uint32)
    recode = np.full(256, 78, np.uint8)
    recode[ASCII] = np.arange(4)
    total = np.zeros((len(rows), 3, 16, 16), np.uint64)
    for coins in product((0, 1), repeat=len(HET_CELLS)):
        tmparr = recode[seqarr]
        for (t, s, code), c in zip(HET_CELLS, coins):
            tmparr[t, s] = ALLELES[code][c]
        total += pooled_literal(oracle, tmparr, tmpmap, sp, K, rows)
    got = pooled_alleles(seqarr, sp, K, rows)
    assert np.array_equal(got.astype(np.uint64) * 2 ** len(HET_CELLS), 16 * total)
    # the heterozygous cells matter: dropping them (as missing) gives other counts
    blind = seqarr.copy()
    for t, s, _ in HET_CELLS:
        blind[t, s] = 78
    assert not np.array_equal(pooled_alleles(blind, sp, K, rows), got)


def test_haplotype_rows():
    seqarr = np.array([[65, 82, 78, 3], [89, 45, 84, 77]], np.uint8)
    assert haplotypes(seqarr).tolist() == [[0, 2, 78, 3], [0, 0, 78, 3], [3, 78, 3, 1], [1, 78, 3, 0]]


def test_without_ambiguity_codes_16_times_the_lineage_model():
    tmparr, tmpmap, sp, _ = synth.simulate_species(5, 2, 300, seed=3, missing=0.15)
    sp[0] = -1
    seqarr, _, _ = synth.make_c5_source(source=(tmparr, tmpmap), ambiguous=0.0)
    rows = np.array(list(combinations(range(5), 4)) + [[0, 0, 1, 2], [3, 3, 3, 3]], np.uint32)
    want = 16 * pooled_factored(tmparr, sp, 5, rows).astype(np.uint64)
    assert np.array_equal(pooled_alleles(seqarr, sp, 5, rows), want)
    # an input already recoded to 0..3 counts the same
    assert np.array_equal(pooled_alleles(tmparr, sp, 5, rows), want)


def test_range_rule_in_lineages():
    # four species of 8 samples are 16 lineages each: 16^4 = 65 536, so S = 65 535 is the last site count in range
    assert species.pooled_range_ok(65_535, [8, 8, 8, 8, 1], alleles=True)
    assert not species.pooled_range_ok(65_536, [8, 8, 8, 8, 1], alleles=True)
    assert species.pooled_range_ok(65_536, [8, 8, 8, 8, 1]) and species.pooled_range_ok(16 * 65_536 - 1, [8, 8, 8, 8])
    # one byte per base: 2n <= 255, i.e. at most 127 samples
    assert species.pooled_range_ok(1, [127, 127, 127, 127], alleles=True)
    assert not species.pooled_range_ok(1, [128, 1, 1, 1], alleles=True)
    assert species.pooled_range_ok(1, [128, 1, 1, 1])
    assert not species.pooled_range_ok(10, [1, 1, 1], alleles=True)


def test_replicate_columns_hand_case():
    spans = np.array([[0, 2], [2, 3], [3, 7], [7, 8]])
    assert replicate_columns(spans, [2, 0, 2, 3]).tolist() == [3, 4, 5, 6, 0, 1, 3, 4, 5, 6, 7]
    assert replicate_columns(spans, np.arange(4)).tolist() == list(range(8))
    assert replicate_columns(spans, [1, 1, 1, 1]).tolist() == [2, 2, 2, 2]


@pytest.mark.parametrize("nquartets", [0, 40])
def test_loop_parameters_recover_the_species_tree(oracle, nquartets):
    """The case of the GPU loop test (tests/test_gpu_species_alleles.py) through the CPU model alone: model matrices of
    every replicate -> oracle scores -> `infer_supertree_exact`.  Every replicate tree, and so the majority-rule tree,
    holds all five splits of the generating species tree, with all 70 species quartets and with 40 sampled ones."""
    from species_alleles_model import LOOP_K, loop_draws, loop_source
    from species_model import parse_tips_newick, score_rows
    from tetrad_amd import qmc
    from tetrad_amd.consensus import Consensus
    seqarr, spans, sp, nwk = loop_source()
    true, tips = parse_tips_newick(nwk)
    assert len(true) == LOOP_K - 3 and tips == frozenset(range(LOOP_K))
    trees = []
    for k, (lidxs, _, _, sq) in enumerate(loop_draws(len(spans), nquartets)):
        cm = pooled_alleles(seqarr, sp, LOOP_K, sq, cols=replicate_columns(spans, lidxs))
        rstat, rscor, zero = score_rows(oracle, cm)
        assert not zero.any()
        trees.append(qmc.infer_supertree_exact(sq, rscor, rstat, LOOP_K, seed=k))
        assert true <= parse_tips_newick(trees[-1])[0]
    with Consensus(LOOP_K) as cons:
        cons.add_newick(trees)
        assert true <= parse_tips_newick(cons.tree(0.5))[0]
