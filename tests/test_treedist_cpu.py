"""CPU-only: the host back end of the tree distance accumulator (`tq_rf_*` with a NULL context) and its Python layer
against the independent model of tests/treedist_model.py.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

import consensus_model as cm
import treedist_model as dm
from tetrad_amd import _lib
from tetrad_amd.consensus import Consensus
from tetrad_amd.treedist import TreeDistances, rf_matrix


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


@pytest.mark.parametrize("T", [4, 5, 6, 12, 33, 63, 64, 65, 100, 127, 128, 129])
def test_arrays_match_the_model(T):
    trees, nsplits, shared, rf, columns = dm.set_model(T, T)
    with TreeDistances(T, len(trees)) as acc:
        acc.add_parents(trees)
        dm.assert_matches(acc, nsplits, shared, rf)
        raw = acc.raw()
        assert [a.dtype for a in raw] == [np.int32, np.uint32, np.uint32] and raw[2].shape == (40, 40)
        assert acc.stats()["columns"] == columns
        assert acc.nsplits().dtype == acc.shared().dtype == acc.rf().dtype == np.int64
        assert nsplits.max() == T - 3 and nsplits[36] == 0            # a binary tree; the star
        assert acc.ndistinct == len(set().union(*(dm.splits(t, T) for t in trees)))


def test_identities():
    T = 33
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    with TreeDistances(T, 64) as acc:
        acc.add_parents(trees)
        n, s, d = acc.nsplits(), acc.shared(), acc.rf()
    assert not np.diag(d).any() and (d == d.T).all() and (s == s.T).all() and (np.diag(s) == n).all()
    for i, j, k in itertools.product(range(40), repeat=3):             # a metric on split sets
        assert d[i, k] <= d[i, j] + d[j, k]
    # the star (tree 36) shares nothing: its distance to tree j is nsplits[j]
    assert n[36] == 0 and (d[36] == n).all() and not s[36].any()
    # tree 0 rooted, unrooted (4) and with unary nodes (8) are one tree
    assert d[0, 4] == d[0, 8] == d[4, 8] == 0 and n[0] == n[4] == n[8] == T - 3


@pytest.mark.parametrize("T", [4, 5, 12, 65])
def test_one_nni_of_a_binary_tree_is_at_distance_two(T):
    rng = np.random.default_rng(T)
    base = cm.unrooted(cm.random_binary(T, rng), T)                     # a root of degree 3: every NNI changes the tree
    moved = [cm.nni(base, T, rng) for _ in range(6)]
    with TreeDistances(T, 7) as acc:
        acc.add_parents([base] + moved)
        assert (acc.rf()[0, 1:] == 2).all() and (acc.shared()[0, 1:] == T - 4).all()
        assert (acc.nsplits() == T - 3).all()


def test_sums_agree_with_the_consensus_counts():
    T = 65
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    with TreeDistances(T, 40) as acc, Consensus(T) as freq:
        acc.add_parents(trees)
        freq.add_parents(trees)
        _, counts, n = freq.splits()
        assert n == 40
        assert int(acc.nsplits().sum()) == int(counts.sum())
        assert int(acc.shared().sum()) == int((counts.astype(np.int64) ** 2).sum())
        assert acc.ndistinct == len(counts) and acc.stats()["columns"] == int((counts >= 2).sum())


def test_accumulation_reads_between_adds_and_reset():
    T = 65
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    with TreeDistances(T, 40) as one, TreeDistances(T, 40) as many:
        one.add_parents(trees)
        many.add_parents(trees[:7])
        many.add_parents([])
        many.add_parents(trees[7:8])
        dm.assert_matches(many, nsplits[:8], shared[:8, :8], rf[:8, :8])   # a read between adds
        dm.assert_matches(many, nsplits[:8], shared[:8, :8], rf[:8, :8])   # and again
        many.add_parents(trees[8:])
        for a, b in zip(many.raw(), one.raw()):
            np.testing.assert_array_equal(a, b)
        dm.assert_matches(many, nsplits, shared, rf)
        many.reset()
        assert many.ntrees == 0 and many.ndistinct == 0 and many.rf().shape == (0, 0) and many.nsplits().shape == (0,)
        many.add_parents(trees[3:9])
        dm.assert_matches(many, nsplits[3:9], shared[3:9, 3:9], rf[3:9, 3:9])
        assert many.stats()["columns"] == dm.expected(trees[3:9], T)[3]


def test_refusals_leave_the_accumulator_unchanged():
    from tetrad_amd._lib import TetradHipError
    T = 12
    trees, nsplits, shared, rf, _ = dm.set_model(T, 3)
    for bad_T in (3, 4097):
        with pytest.raises(TetradHipError, match="T must be 4..4096") as info:
            TreeDistances(bad_T, 4)
        assert info.value.code == -1
    for bad_n in (0, 8193):
        with pytest.raises(TetradHipError, match="max_trees must be 1..8192"):
            TreeDistances(T, bad_n)
    for bad_s in (0, 2 ** 26 + 1):
        with pytest.raises(TetradHipError, match="max_splits must be 1..2\\^26"):
            TreeDistances(T, 4, max_splits=bad_s)
    with TreeDistances(T, 8) as acc:
        acc.add_parents(trees[:5])
        before = acc.raw()
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T                               # two internal nodes point at each other
        with pytest.raises(TetradHipError, match="tq_rf_add: tree 2") as info:
            acc.add_parents([trees[5], trees[6], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8") as info:
            acc.add_parents(trees[5:9])                             # 5 + 4 > 8
        assert info.value.code == -1
        with pytest.raises(ValueError, match="tree 1: 8 taxa"):
            acc.add_newick([dm.newick_of(trees[5], T), dm.newick_of(cm.balanced(8), 8)])
        assert acc.ntrees == 5
        for a, b in zip(acc.raw(), before):
            np.testing.assert_array_equal(a, b)
        dm.assert_matches(acc, nsplits[:5], shared[:5, :5], rf[:5, :5])
        acc.add_parents(trees[5:8])                                 # 8 of 8 fit
        dm.assert_matches(acc, nsplits[:8], shared[:8, :8], rf[:8, :8])


def test_more_distinct_splits_than_max_splits_is_refused_until_a_reset():
    """As `Consensus` does: the add that crosses max_splits fails, every later call fails, a reset makes it usable."""
    from tetrad_amd._lib import TetradHipError
    T = 12
    trees, nsplits, shared, rf, _ = dm.set_model(T, 3)
    distinct = len(dm.splits(trees[0], T) | dm.splits(trees[28], T))
    with TreeDistances(T, 8, max_splits=distinct) as acc:
        acc.add_parents([trees[0], trees[28]])
        dm.assert_matches(acc, nsplits[[0, 28]], shared[np.ix_([0, 28], [0, 28])], rf[np.ix_([0, 28], [0, 28])])
        with pytest.raises(TetradHipError, match="max_splits") as info:
            acc.add_parents([trees[32]])                            # the caterpillar brings new splits
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="reset the accumulator"):
            acc.rf()
        acc.reset()
        acc.add_parents([trees[0], trees[28]])
        dm.assert_matches(acc, nsplits[[0, 28]], shared[np.ix_([0, 28], [0, 28])], rf[np.ix_([0, 28], [0, 28])])


def test_medoid_normalised_and_mean():
    T = 8
    a = cm.unrooted(cm.balanced(T), T)
    b = cm.nni(a, T, np.random.default_rng(0))
    star = cm.star(T)
    with TreeDistances(T, 8) as acc:
        assert acc.mean_rf() == 0.0 and acc.rf_normalized().shape == (0, 0)
        with pytest.raises(ValueError, match="no trees"):
            acc.medoid()
        acc.add_parents([star])
        assert acc.mean_rf() == 0.0 and acc.medoid() == (0, 0) and acc.rf_normalized().tolist() == [[0.0]]
        acc.add_parents([star, a, b, a])                           # star, star, a, b, a
        d, n = acc.rf(), acc.nsplits()
        assert n.tolist() == [0, 0, 5, 5, 5] and d[2, 3] == 2 and d[2, 4] == 0 and d[0, 2] == 5
        norm = acc.rf_normalized()
        assert norm[0, 1] == 0.0 and norm[0, 2] == 1.0 and norm[2, 3] == 0.2 and norm[2, 4] == 0.0
        assert norm.dtype == np.float64 and not np.isnan(norm).any()
        # row sums: the stars 15, a 12, b 14, a 12 -- the tie goes to the lower index
        assert acc.medoid() == (2, 12) and isinstance(acc.medoid()[1], int)
        assert acc.mean_rf() == sum(int(d[i, j]) for i in range(5) for j in range(i + 1, 5)) / 10 == 3.4


def test_rf_matrix_from_newick_with_samples():
    from tetrad_amd.qmc import relabel_tree
    T = 12
    trees, nsplits, shared, rf, _ = dm.set_model(T, 3)
    names = [f"s {t}" if t % 5 == 0 else f"t{t}" for t in range(T)]
    plain = [dm.newick_of(t, T) for t in trees]
    np.testing.assert_array_equal(rf_matrix(plain), rf)
    np.testing.assert_array_equal(rf_matrix([relabel_tree(s, names) for s in plain], samples=names), rf)
    assert rf_matrix(plain[0]).tolist() == [[0]]
    with pytest.raises(ValueError, match="no trees"):
        rf_matrix([])
    with TreeDistances(T, 40, samples=names) as acc:               # the names given at create
        acc.add_newick([relabel_tree(s, names) for s in plain[:6]])
        dm.assert_matches(acc, nsplits[:6], shared[:6, :6], rf[:6, :6])


def test_bootstrap_trees_hands_the_replicates_over(monkeypatch):
    """bootstrap_trees(distances=acc) on the host path: the loop is replaced by its result, the hand-over is real."""
    from tetrad_amd import replicates
    T = 12
    trees, nsplits, shared, rf, _ = dm.set_model(T, 3)
    newicks = [dm.newick_of(t, T) for t in trees[:9]]
    calls = []

    def loop(*args):
        calls.append(args)
        return list(newicks)

    monkeypatch.setattr(replicates, "_bootstrap_trees", loop)
    with TreeDistances(T, 16) as acc, Consensus(T) as freq:
        out = replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9,
                                         distances=acc, consensus=freq)
        assert out == newicks and len(calls) == 1 and freq.ntrees == 9 and acc.ntrees == 9
        dm.assert_matches(acc, nsplits[:9], shared[:9, :9], rf[:9, :9])
        assert replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9) == newicks
        assert acc.ntrees == 9
