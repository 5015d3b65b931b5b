"""CPU: the exact supertree (`tq_stree_*`, host back end).  The row rule is pinned by the
existing `tq_qmc_splits`, the root graph by a NumPy model, and the tree must not depend on the order of the rows or on
how they were added -- which `tq_qmc_tree` cannot promise.  The rest is what any correct implementation must do, on the
inputs of tests/test_qmc_tree.py."""
from itertools import combinations

import numpy as np
import pytest

from supertree_model import (SUM_LIMIT, bad_rows, bipartitions, model_graph, newick_bipartitions, rows_from_tree,
                             sample_quartets)
from tetrad_amd import qmc, synth
from tetrad_amd._lib import TetradHipError
from tetrad_amd.qmc import Supertree, infer_supertree_exact


def distinct(q):
    s = np.sort(q, axis=1)
    return (np.diff(s, axis=1) > 0).all(axis=1)


@pytest.mark.parametrize("weights", [0, 1, 2, 3])
@pytest.mark.parametrize("min_snps,min_ratio", [(0, 1.0), (500, 1.3)])
def test_row_rule_equals_qmc_splits(weights, min_snps, min_ratio):
    """the random rows of test_qmc_tree.py::test_qmc_splits_equal_the_parsed_lines, then scores on 6-decimal rounding
    ties (multiples of 1/128) and weights on 5-decimal ties (strategy 1 on multiples of 1/64): same splits, and
    k == rint(w * 1e5), every row"""
    rng = np.random.default_rng(weights)
    n = 4000
    q = np.sort(rng.integers(0, 60, size=(n, 4)), axis=1).astype(np.uint32)
    sc = rng.gamma(2.0, 20.0, size=(n, 3))
    sc[::37] = 0.001
    sc[5::101, 0] = 0.0
    st = np.stack([rng.integers(0, 3, size=n), rng.integers(0, 3000, size=n)], axis=1).astype(np.uint32)
    ties6 = rng.integers(0, 400 * 128, size=(n, 3)) / 128.0
    ties5 = rng.integers(1, 400 * 64, size=(n, 3)) / 64.0
    ties5[:, 2] = ties5[:, 1]                                   # mean of two equal multiples of 1/64
    ties5[:, 0] = 1.0 / 64.0
    for scores in (sc, ties6, ties5):
        ok = distinct(q)                                        # tq_qmc_splits does not look at the taxa
        sp, w = qmc.qmc_splits(q[ok], scores[ok], st[ok], weights, min_snps, min_ratio)
        want_k = np.rint(w * 1e5).astype(np.uint64)
        assert len(sp) > 100 or (weights == 0 and min_ratio > 1.0)      # strategy 0 has ratio 1: all filtered
        with Supertree(60, n, weights, min_snps, min_ratio) as acc:
            acc.add(q, scores, st)
            got_sp, got_k = acc.rows()
            kept, skipped, sum_k = acc.counts()
        keep = want_k > 0
        np.testing.assert_array_equal(got_sp, sp[keep])
        np.testing.assert_array_equal(got_k, want_k[keep])
        assert kept == keep.sum() and skipped == n - kept and sum_k == int(want_k.sum())
    if weights == 1:                                            # the tie inputs did produce ties
        frac = (ties5[:, 1] * 1e5) % 1.0
        assert (frac == 0.5).sum() > 100


@pytest.mark.parametrize("weights", [0, 1, 2, 3])
def test_bad_rows_are_skipped_and_appear_nowhere(weights):
    rng = np.random.default_rng(9)
    T, n = 30, 700
    q, sc, st, fl = bad_rows(T, n, rng)
    heavy = np.arange(n) % 7 == 6                               # weight >= 4e9 under strategies 1 and 2 only
    with Supertree(T, n, weights) as acc:
        acc.add(q, sc, st, fl)
        sp, k = acc.rows()
        G, B, kept, skipped, sum_k = acc.graph()
    want = 0 if weights in (1, 2) else int(heavy.sum())
    assert kept == want == len(sp) and skipped == n - want
    if want == 0:
        assert sum_k == 0 and not G.any() and not B.any()
    else:
        np.testing.assert_array_equal(np.sort(sp, axis=1), q[heavy])


@pytest.mark.parametrize("T", [4, 5, 16, 128, 129, 300])
def test_root_graph_equals_the_numpy_model(T):
    rng = np.random.default_rng(T)
    n = 3 if T == 4 else 20000
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.3, seed=T)
    n = len(q)
    with Supertree(T, n, weights=1) as acc:
        acc.add(q, sc, st)
        sp, k = acc.rows()
        G, B, kept, skipped, sum_k = acc.graph()
    assert kept == n and skipped == 0 and sum_k == int(k.sum())
    mG, mB = model_graph(sp, k, T)
    np.testing.assert_array_equal(G, mG)
    np.testing.assert_array_equal(B, mB)
    assert B.sum() == 4 * sum_k and G.sum() == 8 * sum_k
    perm = rng.permutation(n)
    cuts = [0, n // 3, n // 2, n]
    with Supertree(T, n, weights=1) as acc:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            acc.add(q[perm][lo:hi], sc[perm][lo:hi], st[perm][lo:hi])
        G2, B2, kept2, _, sum2 = acc.graph()
    assert kept2 == n and sum2 == sum_k
    np.testing.assert_array_equal(G2, G)
    np.testing.assert_array_equal(B2, B)


@pytest.mark.parametrize("T,n,shape,wrong,weights", [(16, 1820, "random", 0.25, 1), (40, 40000, "caterpillar", 0.25, 2),
                                                     (128, 100000, "random", 0.1, 3), (60, 30000, "balanced", 0.4, 0)])
def test_tree_string_is_independent_of_row_order_and_adds(T, n, shape, wrong, weights):
    rng = np.random.default_rng(T + n)
    _, _, q, sc, st = rows_from_tree(T, n, shape, wrong, seed=n)
    ref = infer_supertree_exact(q, sc, st, T, weights=weights, seed=3)
    perm = rng.permutation(n)
    assert infer_supertree_exact(q[perm], sc[perm], st[perm], T, weights=weights, seed=3) == ref
    for pieces in (3, 17):
        with Supertree(T, n, weights) as acc:
            for part in np.array_split(perm[::-1], pieces):
                acc.add(q[part], sc[part], st[part])
            assert acc.tree(3) == ref


@pytest.mark.parametrize("T,seed", [(5, 1), (8, 2), (13, 3), (24, 4), (40, 5)])
def test_recovers_the_generating_tree_from_all_its_quartets(T, seed):
    allq = np.array(list(combinations(range(T), 4)), np.uint32)
    children, root, q, sc, st = rows_from_tree(T, 0, "random", 0.0, seed, quartets=allq)
    truth = bipartitions(children, root, T)
    nwk = infer_supertree_exact(q, sc, st, T, seed=7)
    assert newick_bipartitions(nwk, T) == truth
    assert infer_supertree_exact(q, sc, st, T, seed=7) == nwk              # deterministic in the seed
    for s in (8, 9):
        assert newick_bipartitions(infer_supertree_exact(q, sc, st, T, seed=s), T) == truth


def test_recovers_the_tree_from_a_random_sample_of_quartets():
    T = 30
    quartets = np.sort(synth.random_quartets(T, int(T ** 2.8), seed=3), axis=1)
    children, root, q, sc, st = rows_from_tree(T, 0, "random", 0.0, 11, quartets=quartets)
    assert newick_bipartitions(infer_supertree_exact(q, sc, st, T, seed=1), T) == bipartitions(children, root, T)


def test_weights_outvote_noise():
    """the input of test_qmc_tree.py::test_weights_outvote_noise as rows: 20 % wrong and light (0.05), the rest 1.0"""
    from test_qmc_tree import _bipartitions_from_children, _tree_dist, _true_splits
    T = 16
    rng = np.random.default_rng(21)
    children, root = synth.random_tree_children(T, rng)
    D = _tree_dist(children, root, T)
    quartets = np.array(list(combinations(range(T), 4)), np.uint32)
    splits = _true_splits(D, quartets)
    wrong = rng.random(len(splits)) < 0.2
    topo = np.array([[tuple(s) == (a, b, c, d), tuple(s) == (a, c, b, d), tuple(s) == (a, d, b, c)].index(True)
                     for s, (a, b, c, d) in zip(splits.tolist(), quartets.tolist())])
    topo = np.where(wrong, (topo + 1) % 3, topo).astype(np.uint32)
    n = len(topo)
    sc = np.where(wrong, 0.05, 1.0)[:, None] * np.ones((n, 3))
    sc[np.arange(n), topo] = 0.01
    st = np.stack([topo, np.full(n, 100, np.uint32)], axis=1)
    truth = _bipartitions_from_children(children, root, T)
    with Supertree(T, n, weights=1) as acc:
        acc.add(quartets, sc, st)
        _, k = acc.rows()
        assert sorted(set(k.tolist())) == [5000, 100000]
        assert newick_bipartitions(acc.tree(0), T) == truth
    got = newick_bipartitions(infer_supertree_exact(quartets, sc, st, T, weights=0), T)
    assert len(got & truth) >= len(truth) - 2


def test_degenerate_inputs():
    none = (np.zeros((0, 4), np.uint32), np.zeros((0, 3)), np.zeros((0, 2), np.uint32))
    assert infer_supertree_exact(*none, 1) == "0;"
    assert newick_bipartitions(infer_supertree_exact(*none, 6), 6) == set()                 # a star
    one = (np.array([[0, 1, 2, 3]], np.uint32), np.array([[1.0, 2.0, 3.0]]), np.array([[0, 9]], np.uint32))
    assert newick_bipartitions(infer_supertree_exact(*one, 4), 4) == {frozenset([0, 1])}
    # taxa no quartet mentions still appear exactly once (newick_bipartitions asserts it)
    bips = newick_bipartitions(infer_supertree_exact(*one, 7), 7)
    allt = frozenset(range(7))
    assert any(({0, 1} <= s and not ({2, 3} & s)) or ({0, 1} <= allt - s and not ({2, 3} & (allt - s))) for s in bips)
    for T in (2, 3):
        assert newick_bipartitions(infer_supertree_exact(*none, T), T) == set()


@pytest.mark.parametrize("mode", ["sub", "full"])
@pytest.mark.parametrize("weights", [0, 1, 2, 3])
def test_end_to_end_from_the_reference_rows_of_c1(mode, weights):
    from conftest import load_golden
    from test_qmc_tree import _bipartitions_from_children
    g = load_golden("c1_T16_S5000")
    children, root = synth.random_tree_children(16, np.random.default_rng(synth.CONFIG_SEEDS["c1"]))
    nwk = infer_supertree_exact(g["quartets"], g[f"{mode}_rscor"], g[f"{mode}_rstat"], 16, weights=weights)
    truth = _bipartitions_from_children(children, root, 16)
    assert len(truth) == 13 and newick_bipartitions(nwk, 16) == truth


def test_build_twice_and_seeds():
    _, _, q, sc, st = rows_from_tree(40, 20000, "random", 0.4, seed=6)
    with Supertree(40, len(q), weights=1) as acc:
        acc.add(q, sc, st)
        a, b, c = acc.tree(1), acc.tree(2), acc.tree(1)
        assert a == c and acc.levels >= 3
        assert newick_bipartitions(b, 40) is not None
        assert acc.rows()[0].shape == (len(q), 4)                           # a build leaves the rows intact
        st_ = acc.level_stats()
        assert st_.shape == (acc.levels, 6) and st_[0, 0] == 1 and st_[0, 1] == len(q) and st_[0, 2] == 40 * 39 // 2


def test_c5_shape_sample_with_ten_percent_wrong():
    """T = 128, 400 000 sampled quartets of which 10 % are wrong -> 125 of 125 (DESIGN 4.8's figure for tq_qmc_tree)"""
    T = 128
    children, root, q, sc, st = rows_from_tree(T, 400_000, "random", 0.1, seed=128)
    truth = bipartitions(children, root, T)
    assert len(truth) == 125
    with Supertree(T, len(q)) as acc:
        acc.add(q, sc, st)
        assert newick_bipartitions(acc.tree(1), T) == truth
        assert acc.levels >= 8


def test_range_rule_and_capacity():
    """k = 4e13 per row from strategy 1 (two equal scores of 4e8), single units from scores of 0.00001"""
    big = 40_000_000_000_000
    nbig, rest = divmod(SUM_LIMIT - 1, big)
    T = 12
    q = sample_quartets(T, nbig + 2, np.random.default_rng(0))
    sc = np.tile([1.0, 4.0e8, 4.0e8], (nbig + 2, 1))
    sc[nbig] = [1e-9, rest / 1e5, rest / 1e5]
    sc[nbig + 1] = [1e-9, 1e-5, 1e-5]
    st = np.tile(np.array([0, 7], np.uint32), (nbig + 2, 1))
    with Supertree(T, nbig + 2, weights=1) as acc:
        acc.add(q[:nbig + 1], sc[:nbig + 1], st[:nbig + 1])
        kept, _, sum_k = acc.counts()
        assert kept == nbig + 1 and sum_k == SUM_LIMIT - 1 and 6 * sum_k < 2 ** 53
        assert acc.tree(0).endswith(";")
        acc.add(q[nbig + 1:], sc[nbig + 1:], st[nbig + 1:])
        assert acc.counts()[2] == SUM_LIMIT and 6 * SUM_LIMIT >= 2 ** 53
        with pytest.raises(TetradHipError, match="2\\^53"):
            acc.tree(0)
        assert acc.graph()[4] == SUM_LIMIT                                  # the graph itself is still exact in u64
        with pytest.raises(TetradHipError, match="capacity"):
            acc.add(q[:1], sc[:1], st[:1])
        assert acc.counts()[0] == nbig + 2                                  # refused, not truncated
    with Supertree(T, 5) as acc:
        with pytest.raises(TetradHipError, match="capacity"):
            acc.add(q[:6], sc[:6], st[:6])
        assert acc.counts() == (0, 0, 0)
    with pytest.raises(TetradHipError):
        Supertree(0, 5)
    with pytest.raises(ValueError):
        Supertree(8, 5, weights=4)
