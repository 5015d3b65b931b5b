"""CPU-only: the host back end of the leaf stability accumulator (`tq_ls_*` with a NULL context) and its Python layer
against the independent model of tests/stability_model.py.  Every comparison is exact."""
from math import comb

import numpy as np
import pytest

import consensus_model as cm
import qdist_model as qm
import stability_model as sm
import treedist_model as dm
from tetrad_amd import _lib
from tetrad_amd._lib import TetradHipError
from tetrad_amd.qdist import QuartetDistances
from tetrad_amd.stability import LeafStability, dominant_splits, quartet_frequencies


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def scored(T, trees, quartets, ranks, max_trees=None):
    """(accumulator, counts table) of a `set_model`: all quartets, or the sampled ranks."""
    acc = LeafStability(T, max_trees or len(trees))
    acc.add_parents(trees)
    table = acc.score_all(counts=True) if ranks is None else acc.score_ranks(ranks, counts=True)
    return acc, table


@pytest.mark.parametrize("T", [4, 5, 6, 12, 33, 64, 65, 128, 129])
def test_counts_and_sums_match_the_model_and_obey_the_identities(T):
    trees, quartets, ranks, counts, want = sm.set_model(T, T)
    Q = len(quartets)
    assert Q == (comb(T, 4) if T <= 33 else 3000)
    acc, table = scored(T, trees, quartets, ranks)
    with acc, QuartetDistances(T, 40) as qd:
        sm.assert_matches(acc, table, counts, want, 40)
        assert acc.nquartets == Q
        assert (table.astype(np.int64).sum(axis=1) == 40).all()
        raw = acc.raw().astype(np.int64)
        assert raw[:, 0].sum() == 4 * Q
        qd.add_parents(trees)
        qm.score_model(qd, quartets, ranks)
        assert raw[:, 1].sum() == 4 * qd.resolved().sum()
        n = table[:, :3].astype(np.int64)
        assert (n * n).sum() == qd.raw()[0].astype(np.int64).sum()
        assert (raw[:, 3] <= raw[:, 2]).all() and (raw[:, 2] <= raw[:, 1]).all() and (raw[:, 1] <= 40 * raw[:, 0]).all()
        st = acc.stats()
        assert st["tables"] == 40 and st["table_form"] == 0 and st["workgroups"] == 0 and st["chunks"] == 1


@pytest.mark.parametrize("T", [4, 7, 12])
def test_equal_trees_and_stars_by_hand(T):
    N, each = 9, comb(T - 1, 3)
    tree = cm.random_binary(T, np.random.default_rng(T))
    with LeafStability(T, N) as acc:
        acc.add_parents([tree] * N)
        table = acc.score_all(counts=True)
        assert (acc.raw() == np.array([each, N * each, N * each, N * each], np.uint64)).all()
        assert ((table[:, :3] == N).sum(axis=1) == 1).all() and not table[:, 3].any()
        assert (acc.stability("dif") == 1.0).all() and (acc.stability("res") == 1.0).all()
        acc.reset()
        acc.add_parents([cm.star(T)] * N)
        table = acc.score_all(counts=True)
        assert (acc.raw() == np.array([each, 0, 0, 0], np.uint64)).all()
        assert (table == np.array([0, 0, 0, N], np.uint16)).all()
        assert not acc.stability("max").any()


@pytest.mark.parametrize("T", [6, 9, 12, 33])
def test_one_nni_splits_exactly_the_quartets_across_the_edge(T):
    rng = np.random.default_rng(T)
    base = cm.unrooted(cm.random_binary(T, rng), T)
    for _ in range(4):
        moved = cm.nni(base, T, rng)
        sizes, _ = qm.nni_parts(base, moved, T)
        with LeafStability(T, 2) as acc:
            acc.add_parents([base, moved])
            table = acc.score_all(counts=True).astype(np.int64)
        split = (np.sort(table[:, :3], axis=1) == [0, 1, 1]).all(axis=1) & (table[:, 3] == 0)
        whole = ((table[:, :3] == 2).sum(axis=1) == 1) & (table.sum(axis=1) == 2)
        assert split.sum() == int(np.prod(sizes)) and (split | whole).all()


def test_a_rogue_taxon_ranks_first():
    T = 12
    trees = sm.rogue_set(T)
    N = 2 * T - 5
    assert len(trees) == N == 19
    quartets = qm.all_quartets(T)
    counts, want = sm.expected(trees, T, quartets)
    without = ~(quartets == T - 1).any(axis=1)
    assert ((counts[without][:, :3] == N).sum(axis=1) == 1).all()      # the caterpillar itself never moves
    model = sm.stability(want, N, "dif")
    assert model[T - 1] < model[:T - 1].min()                          # a condition on the input
    names = [f"taxon{t}" for t in range(T)]
    with LeafStability(T, N, samples=names) as acc:
        acc.add_parents(trees)
        table = acc.score_all(counts=True)
        sm.assert_matches(acc, table, counts, want, N)
        assert acc.ranking()[0] == T - 1 and acc.rogues(1) == [names[T - 1]] and acc.rogues(1, "dif") == [names[T - 1]]
        assert acc.ranking().tolist() == sorted(range(T), key=lambda t: (model[t], t))
        assert len(acc.rogues(3, "max")) == 3 and acc.rogues(0) == []
        with pytest.raises(ValueError, match="kind"):
            acc.stability("entropy")
    with LeafStability(T, N) as acc:
        acc.add_parents(trees)
        acc.score_all()
        assert acc.rogues(1) == [T - 1]


def test_order_of_taxa_repeats_and_order_of_calls():
    T = 33
    trees, quartets, ranks, counts, want = sm.set_model(T, T)
    Q = len(quartets)
    rng = np.random.default_rng(1)
    with LeafStability(T, 40) as acc:
        acc.add_parents(trees)
        for perm in ([0, 1, 2, 3], [3, 1, 0, 2], [1, 0, 3, 2], list(rng.permutation(4))):
            table = acc.score(quartets[:5000][:, perm], counts=True)
            np.testing.assert_array_equal(table, sm.permuted_counts(counts[:5000], perm))
            rest = acc.score(quartets[5000:][::-1], counts=True)        # a second call, backwards
            np.testing.assert_array_equal(rest, counts[5000:][::-1])
            np.testing.assert_array_equal(acc.raw().astype(np.int64), want)
            assert acc.nquartets == Q
            acc.clear()                                                 # keeps the trees
            assert acc.ntrees == 40 and acc.nquartets == 0 and not acc.raw().any()
        rows = np.array([row[rng.permutation(4)] for row in quartets[:700]], np.int32)     # another order in every row
        acc.score(rows)
        np.testing.assert_array_equal(acc.raw().astype(np.int64), sm.acc_of(counts[:700], quartets[:700], T))
        acc.clear()
        twice = np.concatenate([quartets[:300], quartets[100:200]])     # rows given twice count twice
        table = acc.score(twice, counts=True)
        np.testing.assert_array_equal(table, np.concatenate([counts[:300], counts[100:200]]))
        np.testing.assert_array_equal(acc.raw().astype(np.int64),
                                      sm.acc_of(counts[:300], quartets[:300], T) + sm.acc_of(counts[100:200], quartets[100:200], T))
        acc.clear()
        k = 12345
        a = acc.score_range(0, k, counts=True)
        b = acc.score_range(k, Q - k, counts=True)
        np.testing.assert_array_equal(np.concatenate([a, b]), counts)
        np.testing.assert_array_equal(acc.raw().astype(np.int64), want)
        acc.clear()
        table = acc.score_ranks(np.arange(Q, dtype=np.uint64), counts=True)     # explicit ranks = the range
        assert acc.score([]) is None and acc.score_ranks([]) is None
        assert acc.score([], counts=True).shape == (0, 4)
        sm.assert_matches(acc, table, counts, want, 40)


def test_more_than_one_host_chunk():
    """101 270 quartets: the host walks them in chunks of 65 536, and the counts array spans both."""
    T = 41
    rng = np.random.default_rng(41)
    trees = [cm.random_binary(T, rng), cm.multifurcating(T, rng), cm.caterpillar(T)]
    quartets = qm.all_quartets(T)
    counts, want = sm.expected(trees, T, quartets)
    with LeafStability(T, 3) as acc:
        acc.add_parents(trees)
        table = acc.score_all(counts=True)
        assert acc.stats()["chunks"] == 2 and acc.stats()["chunk_quartets"] == 65536
        sm.assert_matches(acc, table, counts, want, 3)


def test_score_sample_is_reproducible():
    T = 65
    trees, quartets, ranks, counts, want = sm.set_model(T, T)
    with LeafStability(T, 40) as a, LeafStability(T, 40) as b:
        a.add_parents(trees)
        b.add_parents(trees)
        ra, table = a.score_sample(3000, T, counts=True)
        rb = b.score_sample(3000, T)
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(ra, ranks)
        np.testing.assert_array_equal(a.sample_ranks(3000, T), ranks)
        sm.assert_matches(a, table, counts, want, 40)
        np.testing.assert_array_equal(a.raw(), b.raw())


def test_state_clear_reset_and_empty_scores():
    T = 12
    trees, quartets, ranks, counts, want = sm.set_model(T, 3)
    with LeafStability(T, 40) as acc:
        assert acc.ntrees == 0 and acc.nquartets == 0 and not acc.raw().any()
        for kind in ("dif", "max", "res"):
            assert acc.stability(kind).tolist() == [0.0] * T            # no trees, nothing scored: 0.0, not nan
        # a score without trees is a no-op that leaves a passed array untouched
        mark = np.full((5, 4), 77, np.uint16)
        q = np.ascontiguousarray(quartets[:5], np.int32)
        acc._check(acc._lib.tq_ls_score(acc._h, q.ctypes.data, 5, mark.ctypes.data, None))
        acc._check(acc._lib.tq_ls_score_ranks(acc._h, None, 0, 5, mark.ctypes.data, None))
        assert (mark == 77).all() and acc.nquartets == 0
        acc.add_parents(trees)
        assert acc.stability().tolist() == [0.0] * T                    # trees, but nothing scored
        acc._check(acc._lib.tq_ls_score(acc._h, q.ctypes.data, 0, mark.ctypes.data, None))
        assert (mark == 77).all() and acc.nquartets == 0
        only = quartets[(quartets < 6).all(axis=1)]                     # taxa 6.. are in no scored row
        acc.score(only)
        assert (acc.quartets_per_taxon()[6:] == 0).all() and not acc.stability()[6:].any() and acc.stability("res")[:6].all()
        acc.clear()
        assert acc.ntrees == 40 and acc.nquartets == 0 and not acc.raw().any()
        sm.assert_matches(acc, acc.score_all(counts=True), counts, want, 40)
        acc.reset()
        assert acc.ntrees == 0 and acc.nquartets == 0 and not acc.raw().any()
        assert acc.score_all(counts=True).shape == (comb(T, 4), 4) and acc.nquartets == 0      # no trees: a no-op
        acc.add_parents(trees[3:9])
        w_counts, w_acc = sm.expected(trees[3:9], T, quartets)
        sm.assert_matches(acc, acc.score_all(counts=True), w_counts, w_acc, 6)


def test_refusals_leave_the_accumulator_unchanged():
    T = 12
    trees, quartets, ranks, counts, want = sm.set_model(T, 3)
    for bad_T in (3, 1025):
        with pytest.raises(TetradHipError, match="tq_ls_create: T must be 4..1024") as info:
            LeafStability(bad_T, 4)
        assert info.value.code == -1
    for bad_n in (0, 8193):
        with pytest.raises(TetradHipError, match="tq_ls_create: max_trees must be 1..8192"):
            LeafStability(T, bad_n)
    with LeafStability(T, 8) as acc:
        acc.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T                               # two internal nodes point at each other
        with pytest.raises(TetradHipError, match="tq_ls_add: tree 2") as info:
            acc.add_parents([trees[5], trees[6], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8"):
            acc.add_parents(trees[5:9])                             # 5 + 4 > 8
        assert acc.ntrees == 5
        acc.score(quartets[:100])
        before = acc.raw()
        bad = np.array(quartets[100:110], np.int32)
        bad[7, 2] = bad[7, 0]
        with pytest.raises(TetradHipError, match="tq_ls_score: quartet 7: repeated taxon") as info:
            acc.score(bad, counts=True)
        assert info.value.code == -1
        bad = np.array(quartets[100:110], np.int32)
        bad[3, 3] = T
        with pytest.raises(TetradHipError, match="tq_ls_score: quartet 3: taxon out of range"):
            acc.score(bad)
        bad[3, 3] = -1
        with pytest.raises(TetradHipError, match="quartet 3"):
            acc.score(bad)
        with pytest.raises(TetradHipError, match="tq_ls_score_ranks: rank 2") as info:
            acc.score_ranks([0, 1, comb(T, 4), 2])
        assert info.value.code == -1
        with pytest.raises(ValueError, match="exceeds"):
            acc.score_range(comb(T, 4) - 3, 4)
        with pytest.raises(TetradHipError, match="rank range"):
            acc._check(acc._lib.tq_ls_score_ranks(acc._h, None, comb(T, 4) - 3, 4, None, None))
        with pytest.raises(ValueError, match="shape"):
            acc.score(np.zeros((3, 5), np.int32))
        with pytest.raises(TypeError, match="counts is given by keyword"):
            acc.score(quartets[:3], True)
        with pytest.raises(TetradHipError, match="tq_ls_add: quartets have been scored") as info:
            acc.add_parents(trees[5:6])                             # an add after a score
        assert info.value.code == -1
        assert acc.ntrees == 5 and acc.nquartets == 100
        np.testing.assert_array_equal(acc.raw(), before)
        w_counts, w_acc = sm.expected(trees[:5], T, quartets[:100])
        sm.assert_matches(acc, None, w_counts, w_acc, 5)
        acc.clear()
        acc.add_parents(trees[5:8])                                 # 8 of 8 fit, and adds are allowed again
        w_counts, w_acc = sm.expected(trees[:8], T, quartets)
        sm.assert_matches(acc, acc.score_all(counts=True), w_counts, w_acc, 8)
    with QuartetDistances(T, 4) as qd, pytest.raises(ValueError, match="no counts"):
        qd.score(quartets[:3], counts=True)


def test_dominant_splits_against_the_model():
    T = 12
    trees, quartets, ranks, counts, want = sm.set_model(T, 3)
    n = counts[:, :3]
    top = n.max(axis=1)
    tied = (n == top[:, None]).sum(axis=1) > 1
    assert tied.any() and (~tied).any() and (top[~tied] < 25).any() and (top[~tied] >= 25).any()
    for min_count in (1, 25, 41):
        splits, weights = dominant_splits(quartets, counts.astype(np.uint16), min_count)
        w_splits, w_weights = sm.dominant_splits(quartets, counts, min_count)
        assert splits.dtype == np.uint32 and weights.dtype == np.float64 and splits.shape == (len(weights), 4)
        np.testing.assert_array_equal(splits, w_splits)
        np.testing.assert_array_equal(weights, w_weights)
    assert len(dominant_splits(quartets, counts, 41)[0]) == 0 and len(dominant_splits(quartets, counts)[0]) == (~tied).sum()
    assert dominant_splits([[4, 1, 7, 2]], [[0, 5, 3, 1]])[0].tolist() == [[4, 7, 1, 2]]
    assert dominant_splits([[4, 1, 7, 2]], [[0, 3, 5, 1]])[0].tolist() == [[4, 2, 1, 7]]
    assert dominant_splits([[4, 1, 7, 2]], [[5, 5, 3, 0]])[0].shape == (0, 4)


def test_summary_tree_of_equal_trees_and_frequencies_from_newick():
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.qmc import qmc_tree, relabel_tree
    T = 12
    tree = cm.unrooted(cm.random_binary(T, np.random.default_rng(12)), T)
    text = dm.newick_of(tree, T)
    quartets, counts = quartet_frequencies([text] * 7)
    np.testing.assert_array_equal(quartets, qm.all_quartets(T))
    assert counts.dtype == np.uint16 and ((counts[:, :3] == 7).sum(axis=1) == 1).all()
    summary = qmc_tree(*dominant_splits(quartets, counts), ntaxa=T)
    assert dm.splits(newick_to_parent(summary)[0], T) == dm.splits(tree, T)
    # names through `samples`, explicit rows, one tree as a string
    trees, all_q, ranks, want, _ = sm.set_model(T, 3)
    names = [f"s {t}" if t % 5 == 0 else f"t{t}" for t in range(T)]
    plain = [dm.newick_of(t, T) for t in trees]
    q, c = quartet_frequencies([relabel_tree(s, names) for s in plain], samples=names)
    np.testing.assert_array_equal(c, want)
    sub = all_q[::7]
    q, c = quartet_frequencies(plain[:6], quartets=sub)
    np.testing.assert_array_equal(q, sub)
    np.testing.assert_array_equal(c, sm.expected(trees[:6], T, sub)[0])
    assert quartet_frequencies(plain[0])[1].sum() == comb(T, 4)
    with pytest.raises(ValueError, match="no trees"):
        quartet_frequencies([])
    import tetrad_amd
    assert tetrad_amd.LeafStability is LeafStability and tetrad_amd.dominant_splits is dominant_splits


def test_bootstrap_trees_hands_the_replicates_over(monkeypatch):
    """bootstrap_trees(stability=acc) on the host path: the loop is replaced by its result, the hand-over is real."""
    from tetrad_amd import replicates
    T = 12
    trees, quartets, ranks, counts, want = sm.set_model(T, 3)
    newicks = [dm.newick_of(t, T) for t in trees[:9]]
    calls = []

    def loop(*args):
        calls.append(args)
        return list(newicks)

    monkeypatch.setattr(replicates, "_bootstrap_trees", loop)
    with LeafStability(T, 16) as acc, QuartetDistances(T, 16) as qd:
        out = replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9,
                                         stability=acc, quartet_distances=qd)
        assert out == newicks and len(calls) == 1 and acc.ntrees == 9 and qd.ntrees == 9
        w_counts, w_acc = sm.expected(trees[:9], T, quartets)
        sm.assert_matches(acc, acc.score_all(counts=True), w_counts, w_acc, 9)
        assert replicates.bootstrap_trees(None, np.zeros((T, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 9) == newicks
        assert acc.ntrees == 9 and len(calls) == 2 and len(calls[0]) == len(calls[1])   # the default: the calls of before
