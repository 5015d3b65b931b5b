"""CPU-only: the host back end of the transfer bootstrap accumulator (`tq_tbe_*` with a NULL context) and its Python
layer against the independent model of tests/tbe_model.py.  Every comparison is exact."""
import re

import numpy as np
import pytest

import consensus_model as cm
import tbe_model as tm
from tetrad_amd import _lib
from tetrad_amd.consensus import Consensus
from tetrad_amd.tbe import TransferSupport, percent, transfer_supports


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


# tree_set: 10 base shapes, each followed by 3 perturbations -- the bases are the trees 0, 4, ..., 36:
# rooted, unrooted, with unary nodes, after 1 / 3 / 6 NNIs, with a polytomy, balanced, caterpillar, star
BASES = list(range(0, 40, 4))


@pytest.mark.parametrize("T", [4, 5, 6, 12, 33, 63, 64, 65, 100, 127, 128, 129])
def test_raw_matches_the_model(T):
    for ref in BASES:
        trees, masks, p, phi = tm.set_model(T, T, ref)
        with TransferSupport(T, trees[ref]) as acc:
            got = acc.add_parents(trees, per_tree=True)
            tm.assert_matches(acc, masks, p, phi)
            np.testing.assert_array_equal(got, phi)
            assert got.dtype == np.uint16 and got.shape == (40, len(p))
            if ref == 36:                                          # the star
                assert len(p) == 0 and acc.supports().shape == (0,)
            else:
                assert len(p) >= 1 and (p >= 2).all() and (phi <= p - 1).all()


def test_the_reference_among_its_replicates_and_a_star():
    T = 33
    rng = np.random.default_rng(1)
    ref = cm.random_binary(T, rng)
    with TransferSupport(T, ref) as acc:
        _, p, _ = acc.raw()
        same = acc.add_parents([ref, cm.unrooted(ref, T), cm.with_unary(ref, T, rng)], per_tree=True)
        assert same.shape == (3, T - 3) and not same.any()
        np.testing.assert_array_equal(acc.supports(), np.ones(T - 3))
        np.testing.assert_array_equal(acc.percents(), np.full(T - 3, 100))
        acc.reset()
        stars = acc.add_parents([cm.star(T)] * 2, per_tree=True)
        np.testing.assert_array_equal(stars, np.broadcast_to(p - 1, (2, T - 3)))
        np.testing.assert_array_equal(acc.supports(), np.zeros(T - 3))
        np.testing.assert_array_equal(acc.percents(), np.zeros(T - 3))


def test_one_moved_tip_costs_one_transfer_where_the_frequency_drops_to_zero():
    """The caterpillar ((((0,1),2),3),...,T-1) with tip 2 regrafted beside tip T-1: every branch between the two places
    is gone from the replicate (frequency 0), and every one of them is one moved tip away (phi = 1)."""
    T = 24
    ref = cm.caterpillar(T)
    moved = [int(x) for x in ref]
    u = len(moved)                              # tip 2 leaves a unary node behind; u goes on the edge above tip T - 1
    moved.append(moved[T - 1])
    moved[T - 1] = u
    moved[2] = u
    moved = np.array(moved, np.int32)
    masks, p, want = tm.expected(ref, [moved], T)
    with TransferSupport(T, ref) as acc, Consensus(T) as freq:
        phi = acc.add_parents([moved], per_tree=True)[0]
        freq.add_parents([moved])
        counts, cmasks = freq.support_of(ref)
        np.testing.assert_array_equal(cmasks, acc.raw()[0])
        np.testing.assert_array_equal(phi, want[0])
        assert phi.max() == 1
        np.testing.assert_array_equal(phi == 0, counts == 1)
        assert (counts == 0).sum() >= T // 2
        assert acc.supports().min() >= 1 - 1 / (p.min() - 1) and (acc.supports()[p > 2] > 0).all()


def test_frequency_counts_are_the_replicates_at_distance_zero():
    T = 33
    trees, masks, p, want = tm.set_model(T, 5, 0)
    with TransferSupport(T, trees[0]) as acc, Consensus(T) as freq:
        phi = acc.add_parents(trees, per_tree=True)
        freq.add_parents(trees)
        counts, cmasks = freq.support_of(trees[0])
        np.testing.assert_array_equal(cmasks, masks)
        np.testing.assert_array_equal((phi == 0).sum(axis=0), counts)
        # without the matrix: phi <= p - 1 bounds the sum, so at least `counts` replicates sit at 0
        _, _, phi_sum = acc.raw()
        assert (phi_sum.astype(np.int64) <= (len(trees) - counts) * (p - 1)).all()


def test_accumulation_and_reset():
    T = 65
    trees, masks, p, want = tm.set_model(T, T, 0)
    with TransferSupport(T, trees[0]) as one, TransferSupport(T, trees[0]) as many:
        rows = one.add_parents(trees, per_tree=True)
        np.testing.assert_array_equal(rows.sum(axis=0, dtype=np.uint64), one.raw()[2])
        assert many.add_parents(trees[:7]) is None
        many.add_parents(trees[7:8])
        part = many.add_parents(trees[8:], per_tree=True)
        np.testing.assert_array_equal(part, rows[8:])
        for a, b in zip(many.raw(), one.raw()):
            np.testing.assert_array_equal(a, b)
        assert many.ntrees == one.ntrees == 40
        many.reset()
        got_masks, got_p, got_sum = many.raw()
        np.testing.assert_array_equal(got_masks, masks)
        np.testing.assert_array_equal(got_p, p)
        assert many.ntrees == 0 and not got_sum.any() and not many.supports().any()
        many.add_parents(trees[3:9])
        tm.assert_matches(many, masks, p, want[3:9])
        assert many.add_parents([], per_tree=True).shape == (0, len(p)) and many.ntrees == 6


def test_percents_follow_the_integer_formula():
    T = 4
    ref = cm.balanced(T)
    with TransferSupport(T, ref) as acc:
        acc.add_parents([ref] * 7 + [cm.star(T)])                  # N q = 8, phi_sum = 1: 87.5 percent, rounded half up
        masks, p, phi_sum = acc.raw()
        assert p.tolist() == [2] and phi_sum.tolist() == [1] and acc.supports().tolist() == [0.875]
        assert acc.percents().tolist() == [88] == [tm.percent(1, 2, 8)] == [percent(1, 2, 8)]
        assert re.findall(r"\)(\d+)", acc.map_supports()) == ["88"]
    T = 33
    trees, masks, p, want = tm.set_model(T, T, 0)
    with TransferSupport(T, trees[0]) as acc:
        acc.add_parents(trees)
        _, _, phi_sum = acc.raw()
        assert acc.percents().tolist() == [tm.percent(int(s), int(q), 40) for s, q in zip(phi_sum, p)]
        np.testing.assert_allclose(acc.supports(), 1 - want.sum(axis=0) / (40 * (p - 1)), rtol=0, atol=1e-15)
        assert percent(0, 5, 0) == 0 and not TransferSupport(T, trees[0]).percents().any()


def test_map_supports_places_the_labels_where_the_consensus_does():
    T = 12
    trees, masks, p, want = tm.set_model(T, 3, 0)
    names = [f"s {t}" if t % 5 == 0 else f"t{t}" for t in range(T)]
    from tetrad_amd.qmc import relabel_tree
    for samples, text in ((None, tm.newick_of(trees[0], T)), (names, relabel_tree(tm.newick_of(trees[0], T), names))):
        with TransferSupport(T, text, samples) as acc, Consensus(T) as freq:
            acc.add_parents(trees)
            freq.add_parents(trees)
            ours, theirs = acc.map_supports(), freq.map_supports(text, samples)
            assert re.sub(r"\)\d+", ")#", ours) == re.sub(r"\)\d+", ")#", theirs) and ours.count(")") == T - 1
            assert len(re.findall(r"\)\d+", ours)) == T - 3
            assert sorted(int(x) for x in re.findall(r"\)(\d+)", ours)) == sorted(acc.percents().tolist())
            acc.reset()
            freq.reset()
            acc.add_parents([trees[0]] * 3)                         # every branch in every replicate: both write 100
            freq.add_parents([trees[0]] * 3)
            assert acc.map_supports() == freq.map_supports(text, samples)
    with TransferSupport(T, trees[0]) as acc:                      # a parent array as reference: numeric tips
        acc.add_parents(trees)
        by_array = acc.map_supports()
        assert by_array == acc.map_supports(tm.newick_of(trees[0], T))
        assert by_array == transfer_supports(tm.newick_of(trees[0], T), [tm.newick_of(t, T) for t in trees])
        with pytest.raises(ValueError, match="branches of the reference"):
            acc.map_supports(tm.newick_of(trees[28], T))


def test_refusals_leave_the_accumulator_unchanged():
    from tetrad_amd._lib import TetradHipError
    T = 12
    trees, masks, p, want = tm.set_model(T, 3, 0)
    for bad_T in (3, 4097):
        with pytest.raises(TetradHipError, match="T must be 4..4096") as info:
            TransferSupport(bad_T, cm.star(bad_T))
        assert info.value.code == -1
    with pytest.raises(TetradHipError, match="tq_tbe_create") as info:
        TransferSupport(T, np.array([T] * (T - 1) + [-1, -1], np.int32))       # taxon T - 1 is a second root
    assert info.value.code == -1
    with pytest.raises(ValueError, match="taxa"):
        TransferSupport(T, tm.newick_of(cm.balanced(8), 8))
    with TransferSupport(T, trees[0]) as acc:
        acc.add_parents(trees[:5])
        before = acc.raw()
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T                               # two internal nodes point at each other
        with pytest.raises(TetradHipError, match="tq_tbe_add: tree 2") as info:
            acc.add_parents([trees[5], trees[6], cyc, trees[7]], per_tree=True)
        assert info.value.code == -1
        with pytest.raises(ValueError, match="tree 1: 8 taxa"):
            acc.add_newick([tm.newick_of(trees[5], T), tm.newick_of(cm.balanced(8), 8)])
        assert acc.ntrees == 5
        for a, b in zip(acc.raw(), before):
            np.testing.assert_array_equal(a, b)
        tm.assert_matches(acc, masks, p, want[:5])


def test_bootstrap_trees_hands_the_replicates_over(monkeypatch):
    """bootstrap_trees(transfer=acc) on the host path: the loop is replaced by its result, the hand-over is real."""
    from tetrad_amd import replicates
    T = 12
    trees, masks, p, want = tm.set_model(T, 3, 0)
    newicks = [tm.newick_of(t, T) for t in trees[:9]]
    calls = []

    def loop(*args):
        calls.append(args)
        return list(newicks)

    monkeypatch.setattr(replicates, "_bootstrap_trees", loop)
    with TransferSupport(T, trees[0]) as acc, TransferSupport(T, trees[0]) as hand, Consensus(T) as freq:
        out = replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9,
                                         transfer=acc, consensus=freq)
        assert out == newicks and len(calls) == 1 and freq.ntrees == 9
        hand.add_newick(out)
        for a, b in zip(acc.raw(), hand.raw()):
            np.testing.assert_array_equal(a, b)
        tm.assert_matches(acc, masks, p, want[:9])
        assert replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9) == newicks
        assert acc.ntrees == 9
