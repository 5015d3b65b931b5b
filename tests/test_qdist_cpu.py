"""CPU-only: the host back end of the quartet distance accumulator (`tq_qd_*` with a NULL context) and its Python layer
against the independent model of tests/qdist_model.py.  Every comparison is exact."""
import ctypes
import itertools
from math import comb

import numpy as np
import pytest

import consensus_model as cm
import qdist_model as qm
import treedist_model as dm
from tetrad_amd import _lib
from tetrad_amd.qdist import QuartetDistances, quartet_distance_matrix


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def scored(T, trees, quartets, ranks, max_trees=None):
    acc = QuartetDistances(T, max_trees or len(trees))
    acc.add_parents(trees)
    qm.score_model(acc, quartets, ranks)
    return acc


@pytest.mark.parametrize("T", [4, 5, 6, 12, 33, 64, 65, 128, 129])
def test_classes_match_the_model_and_obey_the_identities(T):
    trees, quartets, ranks, *classes = qm.set_model(T, T)
    Q = len(quartets)
    assert Q == (comb(T, 4) if T <= 33 else 3000)
    with scored(T, trees, quartets, ranks) as acc:
        qm.assert_matches(acc, classes, Q)
        same, both = acc.raw()
        assert same.dtype == both.dtype == np.uint64 and same.shape == both.shape == (40, 40)
        A, B, C, D, E = acc.counts()
        res = acc.resolved()
        assert (A + B + C + D + E == Q).all()
        assert (A == A.T).all() and (B == B.T).all() and (E == E.T).all() and (C == D.T).all()
        assert (np.diag(A) == res).all() and not np.diag(B).any() and not np.diag(C).any() and not np.diag(D).any()
        assert min(A.min(), B.min(), C.min(), D.min(), E.min()) >= 0
        # tree 0 rooted, with its root dissolved (4) and with unary nodes (8) are one tree; a binary tree resolves
        # every quartet; the star (36) none
        d = acc.distance()
        assert d[0, 4] == d[0, 8] == d[4, 8] == 0 and res[0] == res[4] == res[8] == Q
        assert res[36] == 0 and E[36, 36] == Q and (D[36] == res).all() and (d[36] == res).all()
        st = acc.stats()
        assert st["tables"] == 40 and st["table_form"] == 0 and st["kslices"] == 0


def test_triangle_inequality():
    T = 12
    trees, quartets, ranks, *classes = qm.set_model(T, T)
    with scored(T, trees, quartets, ranks) as acc:
        d = acc.distance()
    for i, j, k in itertools.product(range(40), repeat=3):
        assert d[i, k] <= d[i, j] + d[j, k]


@pytest.mark.parametrize("T", [6, 9, 12, 33])
def test_one_nni_and_one_contraction_count_the_quartets_across_the_edge(T):
    """A binary tree, one NNI of it over an edge with subtrees of a, b, c, d taxa, and the tree with that edge
    contracted: exactly the a b c d quartets with one taxon in each subtree change."""
    rng = np.random.default_rng(T)
    base = cm.unrooted(cm.random_binary(T, rng), T)                 # a root of degree 3: every NNI changes the tree
    for _ in range(4):
        moved = cm.nni(base, T, rng)
        sizes, side = qm.nni_parts(base, moved, T)
        n = int(np.prod(sizes))
        flat = qm.contract(base, T, side)
        assert len(dm.splits(flat, T)) == T - 4
        with QuartetDistances(T, 3) as acc:
            acc.add_parents([base, moved, flat])
            acc.score_all()
            A, B, C, D, E = acc.counts()
            Q = comb(T, 4)
            assert B[0, 1] == n and C[0, 1] == D[0, 1] == E[0, 1] == 0 and A[0, 1] == Q - n
            assert C[0, 2] == n and B[0, 2] == D[0, 2] == E[0, 2] == 0 and A[0, 2] == Q - n
            assert B[1, 2] == 0 and C[1, 2] == n and acc.distance()[0, 1] == n
            assert acc.resolved().tolist() == [Q, Q, Q - n]
            qm.assert_matches(acc, qm.expected([base, moved, flat], T, qm.all_quartets(T)), Q)


def test_more_than_one_host_chunk():
    """101 270 quartets: the host walks them in chunks of 65 536."""
    T = 41
    rng = np.random.default_rng(41)
    trees = [cm.random_binary(T, rng), cm.multifurcating(T, rng), cm.caterpillar(T)]
    with QuartetDistances(T, 3) as acc:
        acc.add_parents(trees)
        acc.score_all()
        assert acc.stats()["chunks"] == 2 and acc.stats()["chunk_quartets"] == 65536
        qm.assert_matches(acc, qm.expected(trees, T, qm.all_quartets(T)), comb(T, 4))


def test_order_of_taxa_and_of_calls_do_not_matter():
    T = 33
    trees, quartets, ranks, *classes = qm.set_model(T, T)
    Q = len(quartets)
    rng = np.random.default_rng(1)
    shuffled = np.array([row[rng.permutation(4)] for row in quartets[:5000]], np.int32)
    with scored(T, trees, quartets, ranks) as one, QuartetDistances(T, 40) as acc:
        want = one.raw()
        acc.add_parents(trees)
        acc.score(shuffled)
        acc.score(quartets[5000:][::-1])                           # two calls, the second backwards
        assert acc.nquartets == Q
        for a, b in zip(acc.raw(), want):
            np.testing.assert_array_equal(a, b)
        acc.clear()                                                 # keeps the trees
        assert acc.ntrees == 40 and acc.nquartets == 0 and not acc.raw()[0].any() and not acc.raw()[1].any()
        k = 12345
        acc.score_range(0, k)
        acc.score_range(k, Q - k)
        for a, b in zip(acc.raw(), want):
            np.testing.assert_array_equal(a, b)
        acc.clear()
        acc.score_ranks(np.arange(Q, dtype=np.uint64))              # explicit ranks = the range
        acc.score([])
        acc.score_ranks([])
        for a, b in zip(acc.raw(), want):
            np.testing.assert_array_equal(a, b)
        acc.reset()                                                 # forgets the trees
        assert acc.ntrees == 0 and acc.nquartets == 0 and acc.raw()[0].shape == (0, 0)
        acc.score_all()                                             # no trees: a no-op
        assert acc.nquartets == 0
        acc.add_parents(trees[3:9])
        acc.score_all()
        qm.assert_matches(acc, [c[3:9, 3:9] for c in classes], Q)


def test_score_sample_is_reproducible():
    T = 65
    trees, quartets, ranks, *classes = qm.set_model(T, T)
    with QuartetDistances(T, 40) as a, QuartetDistances(T, 40) as b:
        a.add_parents(trees)
        b.add_parents(trees)
        ra, rb = a.score_sample(3000, T), b.score_sample(3000, T)
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(ra, ranks)                    # the model drew the same way
        assert ra.dtype == np.uint64 and (np.diff(ra.astype(np.int64)) > 0).all()
        qm.assert_matches(a, classes, 3000)
        for x, y in zip(a.raw(), b.raw()):
            np.testing.assert_array_equal(x, y)
        assert not np.array_equal(a.sample_ranks(3000, T + 1), ra)
        with pytest.raises(ValueError, match="distinct"):
            a.sample_ranks(comb(T, 4) + 1, 0)


def test_refusals_leave_the_accumulator_unchanged():
    from tetrad_amd._lib import TetradHipError
    T = 12
    trees, quartets, ranks, *classes = qm.set_model(T, 3)
    for bad_T in (3, 1025):
        with pytest.raises(TetradHipError, match="T must be 4..1024") as info:
            QuartetDistances(bad_T, 4)
        assert info.value.code == -1
    for bad_n in (0, 8193):
        with pytest.raises(TetradHipError, match="max_trees must be 1..8192"):
            QuartetDistances(T, bad_n)
    with QuartetDistances(T, 8) as acc:
        acc.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T                               # two internal nodes point at each other
        with pytest.raises(TetradHipError, match="tq_qd_add: tree 2") as info:
            acc.add_parents([trees[5], trees[6], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8"):
            acc.add_parents(trees[5:9])                             # 5 + 4 > 8
        with pytest.raises(ValueError, match="tree 1: 8 taxa"):
            acc.add_newick([dm.newick_of(trees[5], T), dm.newick_of(cm.balanced(8), 8)])
        assert acc.ntrees == 5
        acc.score(quartets[:100])
        before = acc.raw()
        bad = np.array(quartets[100:110], np.int32)
        bad[7, 2] = bad[7, 0]
        with pytest.raises(TetradHipError, match="tq_qd_score: quartet 7: repeated taxon") as info:
            acc.score(bad)
        assert info.value.code == -1
        bad = np.array(quartets[100:110], np.int32)
        bad[3, 3] = T
        with pytest.raises(TetradHipError, match="tq_qd_score: quartet 3: taxon out of range"):
            acc.score(bad)
        bad[3, 3] = -1
        with pytest.raises(TetradHipError, match="quartet 3"):
            acc.score(bad)
        with pytest.raises(TetradHipError, match="tq_qd_score_ranks: rank 2") as info:
            acc.score_ranks([0, 1, comb(T, 4), 2])
        assert info.value.code == -1
        with pytest.raises(ValueError, match="exceeds"):
            acc.score_range(comb(T, 4) - 3, 4)
        with pytest.raises(TetradHipError, match="rank range"):
            acc._check(acc._lib.tq_qd_score_ranks(acc._h, None, comb(T, 4) - 3, 4, None))
        with pytest.raises(ValueError, match="shape"):
            acc.score(np.zeros((3, 5), np.int32))
        with pytest.raises(TetradHipError, match="quartets have been scored") as info:
            acc.add_parents(trees[5:6])                             # an add after a score
        assert info.value.code == -1
        assert acc.ntrees == 5 and acc.nquartets == 100
        for a, b in zip(acc.raw(), before):
            np.testing.assert_array_equal(a, b)
        qm.assert_matches(acc, qm.expected(trees[:5], T, quartets[:100]), 100)
        acc.clear()
        acc.add_parents(trees[5:8])                                 # 8 of 8 fit, and adds are allowed again
        acc.score_all()
        qm.assert_matches(acc, [c[:8, :8] for c in classes], len(quartets))


def test_medoid_normalised_and_mean():
    T = 8
    a = cm.unrooted(cm.balanced(T), T)
    b = cm.nni(a, T, np.random.default_rng(0))
    star = cm.star(T)
    n = int(np.prod(qm.nni_parts(a, b, T)[0]))
    with QuartetDistances(T, 8) as acc:
        assert acc.mean_distance() == 0.0 and acc.normalized().shape == (0, 0)
        with pytest.raises(ValueError, match="no trees"):
            acc.medoid()
        acc.add_parents([star])
        assert acc.normalized().tolist() == [[0.0]] and acc.nquartets == 0     # nothing scored: 0.0, not nan
        assert acc.mean_distance() == 0.0 and acc.medoid() == (0, 0)
        acc.add_parents([star, a, b, a])                           # star, star, a, b, a
        assert acc.normalized().tolist() == [[0.0] * 5] * 5
        acc.score_all()
        d = acc.distance()
        assert d[0, 1] == 0 and d[0, 2] == 70 and d[2, 3] == n and d[2, 4] == 0 and d.dtype == np.int64
        norm = acc.normalized()
        assert norm.dtype == np.float64 and norm[0, 2] == 1.0 and norm[2, 3] == n / 70 and norm[2, 4] == 0.0
        # row sums: the stars 210, a 140 + n, b 140 + 2 n, a 140 + n -- the tie goes to the lower index
        assert acc.medoid() == (2, 140 + n) and isinstance(acc.medoid()[1], int)
        assert acc.mean_distance() == sum(int(d[i, j]) for i in range(5) for j in range(i + 1, 5)) / 10


def test_word_rule_is_exported(lib):
    rng = np.random.default_rng(5)
    for _ in range(50):
        code = rng.integers(0, 4, size=(2, 64))
        x = [sum(1 << b for b in range(64) if code[0, b] == k) for k in range(3)]
        y = [sum(1 << b for b in range(64) if code[1, b] == k) for k in range(3)]
        same, both = ctypes.c_uint32(), ctypes.c_uint32()
        lib.tq_qd_word_counts(*x, *y, ctypes.byref(same), ctypes.byref(both))
        assert same.value == int(((code[0] == code[1]) & (code[0] < 3)).sum())
        assert both.value == int(((code[0] < 3) & (code[1] < 3)).sum())


def test_matrix_from_newick_with_samples():
    from tetrad_amd.qmc import relabel_tree
    T = 12
    trees, quartets, ranks, A, B, C, D, E = qm.set_model(T, 3)
    dist = B + C + D
    names = [f"s {t}" if t % 5 == 0 else f"t{t}" for t in range(T)]
    plain = [dm.newick_of(t, T) for t in trees]
    np.testing.assert_array_equal(quartet_distance_matrix(plain), dist)
    np.testing.assert_array_equal(quartet_distance_matrix([relabel_tree(s, names) for s in plain], samples=names), dist)
    sub = quartets[::7]
    np.testing.assert_array_equal(quartet_distance_matrix(plain[:6], quartets=sub),
                                  sum(qm.expected(trees[:6], T, sub)[1:4]))
    assert quartet_distance_matrix(plain[0]).tolist() == [[0]]
    with pytest.raises(ValueError, match="no trees"):
        quartet_distance_matrix([])
    import tetrad_amd
    assert tetrad_amd.QuartetDistances is QuartetDistances


def test_bootstrap_trees_hands_the_replicates_over(monkeypatch):
    """bootstrap_trees(quartet_distances=acc) on the host path: the loop is replaced by its result, the hand-over is
    real."""
    from tetrad_amd import replicates
    from tetrad_amd.treedist import TreeDistances
    T = 12
    trees, quartets, ranks, *classes = qm.set_model(T, 3)
    newicks = [dm.newick_of(t, T) for t in trees[:9]]
    calls = []

    def loop(*args):
        calls.append(args)
        return list(newicks)

    monkeypatch.setattr(replicates, "_bootstrap_trees", loop)
    with QuartetDistances(T, 16) as acc, TreeDistances(T, 16) as rf:
        out = replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9,
                                         quartet_distances=acc, distances=rf)
        assert out == newicks and len(calls) == 1 and rf.ntrees == 9 and acc.ntrees == 9
        acc.score_all()
        qm.assert_matches(acc, [c[:9, :9] for c in classes], len(quartets))
        assert replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9) == newicks
        assert acc.ntrees == 9 and len(calls) == 2 and len(calls[0]) == len(calls[1])   # the default: the calls of before
