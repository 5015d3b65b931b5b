"""GPU: the device execution of the leaf stability accumulator (`tq_ls_*` with a context: `tq_fit_table_kernel` at an
add; `tq_unrank_kernel`, `tq_qd_encode_kernel`, `tq_ls_count_kernel` per chunk of quartets) equals the host back end and
the independent model of tests/stability_model.py bit for bit, the per-taxon sums and the counts table both -- across both
table forms, the staged tile of trees, the word and workgroup boundaries of the planes, the largest LDS accumulator,
quartet chunks, explicit rows, streams, repeated reads, clears, resets, and in the replicate loop."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest

import consensus_model as cm
import qdist_model as qm
import stability_model as sm
import treedist_model as dm
from tetrad_amd.qdist import QuartetDistances
from tetrad_amd.stability import LeafStability

pytestmark = pytest.mark.gpu

GROUP = 16 * 64             # quartets of one workgroup of the count kernel: 16 plane words


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def tile(engine):
    """The trees tq_ls_count_kernel stages per pass, as the binding reports it."""
    with LeafStability(4, 1, engine=engine) as acc:
        value = acc.stats()["tree_tile"]
    assert 2 <= value <= 64
    return value


def assert_same(dev, host):
    np.testing.assert_array_equal(dev.raw(), host.raw())
    assert dev.ntrees == host.ntrees and dev.nquartets == host.nquartets


@pytest.mark.parametrize("T", [4, 5, 33, 128, 129])
def test_device_equals_host_and_model(engine, T):
    """40 trees; the table in LDS up to 128 taxa, through L2 above."""
    trees, quartets, ranks, counts, want = sm.set_model(T, T)
    with LeafStability(T, 40, engine=engine) as dev, LeafStability(T, 40) as host:
        tables = []
        for acc in (dev, host):
            acc.add_parents(trees)
            tables.append(acc.score_all(counts=True) if ranks is None else acc.score_ranks(ranks, counts=True))
        sm.assert_matches(dev, tables[0], counts, want, 40)
        np.testing.assert_array_equal(tables[0], tables[1])
        assert_same(dev, host)
        st = dev.stats()
        assert st["table_form"] == (1 if T <= 128 else 2) and st["tables"] == 40 and st["chunks"] == 1
        assert st["workgroups"] == -(-len(quartets) // GROUP)


PAIRS_T, PAIRS_Q = 33, 5000


@lru_cache(maxsize=None)
def pairs_model():
    """65 independent random binary trees, each followed by one NNI of itself, over 5 000 sampled quartets: 79 plane
    words, 4 full workgroups of the count kernel and one of 15 words."""
    trees = dm.nni_pairs(PAIRS_T, 65, PAIRS_T)
    ranks = qm.sample_ranks(PAIRS_T, PAIRS_Q, PAIRS_T)
    quartets = qm.unrank(ranks, PAIRS_T)
    code = sm.code_array(trees, PAIRS_T, quartets)
    code.setflags(write=False)
    return trees, quartets, ranks, code


def pairs_expected(N, lo=0, hi=PAIRS_Q):
    trees, quartets, ranks, code = pairs_model()
    counts = sm.counts_of(code[:N, lo:hi])
    return counts, sm.acc_of(counts, quartets[lo:hi], PAIRS_T)


@pytest.mark.parametrize("which", ["one", "tile - 1", "tile", "tile + 1", "130"])
def test_trees_against_the_staged_tile(engine, tile, which):
    N = {"one": 1, "tile - 1": tile - 1, "tile": tile, "tile + 1": tile + 1, "130": 130}[which]
    trees, quartets, ranks, _ = pairs_model()
    counts, want = pairs_expected(N)
    with LeafStability(PAIRS_T, N, engine=engine) as dev:
        dev.add_parents(trees[:N])
        table = dev.score_ranks(ranks, counts=True)
        sm.assert_matches(dev, table, counts, want, N)
        sm.assert_matches(dev, None, counts, want, N)               # a second read
        assert dev.stats()["chunk_words"] >= 79 and dev.stats()["chunks"] == 1 and dev.stats()["tree_tile"] == tile


@pytest.mark.parametrize("Q", [1, 63, 64, 65, GROUP - 1, GROUP, GROUP + 1, PAIRS_Q])
def test_word_and_workgroup_boundaries(engine, Q):
    """The last partial word, the last partial group of 16 words, and one quartet past each."""
    trees, quartets, ranks, _ = pairs_model()
    counts, want = pairs_expected(40, 0, Q)
    with LeafStability(PAIRS_T, 40, engine=engine) as dev:
        dev.add_parents(trees[:40])
        table = dev.score_ranks(ranks[:Q], counts=True)
        sm.assert_matches(dev, table, counts, want, 40)
        assert dev.nquartets == Q and dev.stats()["workgroups"] == -(-(-(-Q // 64)) // 16)
        dev.clear()
        dev.score_ranks(ranks[:Q])                                  # without the counts array
        sm.assert_matches(dev, None, counts, want, 40)


def test_largest_lds_accumulator(engine):
    """1 024 taxa: 32 KiB of per-workgroup sums; a caterpillar (depths up to 1 023), a balanced and a random tree."""
    T = 1024
    rng = np.random.default_rng(T)
    trees = [cm.caterpillar(T), cm.balanced(T), cm.random_binary(T, rng)]
    ranks = qm.sample_ranks(T, 2000, T)
    with LeafStability(T, 3, engine=engine) as dev, LeafStability(T, 3) as host:
        tables = []
        for acc in (dev, host):
            acc.add_parents(trees)
            tables.append(acc.score_ranks(ranks, counts=True))
        np.testing.assert_array_equal(tables[0], tables[1])
        assert_same(dev, host)
        assert dev.stats()["table_form"] == 2 and dev.stats()["workgroups"] == 2
        raw = dev.raw().astype(np.int64)
        assert raw[:, 0].sum() == 4 * 2000 and (raw[:, 1] == 3 * raw[:, 0]).all() and not tables[0][:, 3].any()


def test_quartet_chunks(engine):
    """A scratch budget of 100 000 bytes with room for 65 trees: 64 x 56 + 65 x 24 = 5 144 bytes per plane word, 19 words,
    1 216 quartets, 5 chunks of 5 000; the counts array spans the chunks."""
    trees, quartets, ranks, _ = pairs_model()
    counts, want = pairs_expected(65)
    engine.set_option("qdist_scratch_bytes", 100_000)
    try:
        small = LeafStability(PAIRS_T, 65, engine=engine)
    finally:
        engine.set_option("qdist_scratch_bytes", 0)
    with small, LeafStability(PAIRS_T, 65, engine=engine) as one:
        tables = []
        for acc in (small, one):
            acc.add_parents(trees[:65])
            tables.append(acc.score_ranks(ranks, counts=True))
        sm.assert_matches(small, tables[0], counts, want, 65)
        np.testing.assert_array_equal(tables[0], tables[1])
        assert_same(small, one)
        assert small.stats()["chunk_quartets"] == 1216 and small.stats()["chunks"] == 5 and one.stats()["chunks"] == 1
        assert small.stats()["workgroups"] == 1 and one.stats()["workgroups"] == 5     # the last chunk: 136 quartets
        small.clear()
        table = small.score(quartets, counts=True)                  # the explicit array in chunks too
        assert small.stats()["chunks"] == 10
        sm.assert_matches(small, table, counts, want, 65)
        small.clear()
        one.clear()
        a, b = small.score_range(100, 4000, counts=True), one.score_range(100, 4000, counts=True)     # and a range
        np.testing.assert_array_equal(a, b)
        assert_same(small, one)
        w_counts, w_acc = sm.expected(trees[:65], PAIRS_T, qm.all_quartets(PAIRS_T)[100:4100])
        sm.assert_matches(small, a, w_counts, w_acc, 65)
        small.clear()
        small.score_ranks(ranks)                                    # in flight, no counts array
        sm.assert_matches(small, None, counts, want, 65)


def test_explicit_rows_in_any_order_and_repeated(engine):
    trees, quartets, ranks, _ = pairs_model()
    counts, want = pairs_expected(40)
    rng = np.random.default_rng(2)
    with LeafStability(PAIRS_T, 40, engine=engine) as dev:
        dev.add_parents(trees[:40])
        for perm in ([2, 0, 3, 1], [3, 2, 1, 0]):
            table = dev.score(quartets[:, perm], counts=True)
            np.testing.assert_array_equal(table, sm.permuted_counts(counts, perm))
            np.testing.assert_array_equal(dev.raw().astype(np.int64), want)
            dev.clear()
        dev.score(np.array([row[rng.permutation(4)] for row in quartets], np.int32))      # another order in every row
        np.testing.assert_array_equal(dev.raw().astype(np.int64), want)
        table = dev.score(quartets[1000:1100], counts=True)         # rows given twice count twice
        np.testing.assert_array_equal(table, counts[1000:1100])
        np.testing.assert_array_equal(dev.raw().astype(np.int64), want + sm.acc_of(counts[1000:1100], quartets[1000:1100], PAIRS_T))
        assert dev.nquartets == PAIRS_Q + 100


def test_streams_reads_between_scores_clear_and_reset(engine):
    import torch
    trees, quartets, ranks, _ = pairs_model()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    N = 70
    counts, want = pairs_expected(N)
    with LeafStability(PAIRS_T, N, engine=engine) as dev:
        dev.add_parents(trees[:30], stream=s1.cuda_stream)
        dev.add_parents(trees[30:N], stream=s2.cuda_stream)
        tables = []
        for i, lo in enumerate(range(0, PAIRS_Q, 700)):             # scores alternating between two streams
            tables.append(dev.score_ranks(ranks[lo:lo + 700], stream=(s1, s2)[i % 2].cuda_stream, counts=i % 3 == 0))
        sm.assert_matches(dev, None, counts, want, N)
        np.testing.assert_array_equal(tables[0], counts[:700])
        np.testing.assert_array_equal(tables[3], counts[2100:2800])
        assert tables[1] is None
        dev.clear()                                                 # keeps the trees
        assert dev.ntrees == N and dev.nquartets == 0 and not dev.raw().any()
        dev.score_ranks(ranks[:2000])
        sm.assert_matches(dev, None, *pairs_expected(N, 0, 2000), N)                # score, read,
        dev.score_ranks(ranks[2000:])
        sm.assert_matches(dev, None, counts, want, N)               # score, read
        dev.reset()
        assert dev.ntrees == 0 and not dev.raw().any()
        mark = dev.score_ranks(ranks, counts=True)                  # no trees: a no-op
        assert dev.nquartets == 0 and not mark.any() and not dev.raw().any()
        dev.add_parents(trees[33:39])                               # a smaller set, nothing stale
        w_counts, w_acc = sm.expected(trees[33:39], PAIRS_T, quartets)
        sm.assert_matches(dev, dev.score_ranks(ranks, counts=True), w_counts, w_acc, 6)
    torch.cuda.synchronize()


def test_stars_and_equal_trees(engine):
    T, Q = 33, comb(33, 4)
    each = comb(T - 1, 3)
    tree = cm.random_binary(T, np.random.default_rng(7))
    with LeafStability(T, 80, engine=engine) as dev:
        dev.add_parents([cm.star(T)] * 3)
        table = dev.score_all(counts=True)
        assert (table == np.array([0, 0, 0, 3], np.uint16)).all() and len(table) == Q
        assert (dev.raw() == np.array([each, 0, 0, 0], np.uint64)).all()
        dev.reset()
        dev.add_parents([tree] * 70)                                # every tile of trees sets the same bits
        table = dev.score_all(counts=True)
        assert ((table[:, :3] == 70).sum(axis=1) == 1).all() and not table[:, 3].any()
        assert (dev.raw() == np.array([each, 70 * each, 70 * each, 70 * each], np.uint64)).all()
        assert (dev.stability("dif") == 1.0).all()


def test_refusals_leave_the_device_state_unchanged(engine):
    from tetrad_amd._lib import TetradHipError
    T = PAIRS_T
    trees, quartets, ranks, _ = pairs_model()
    with LeafStability(T, 8, engine=engine) as dev:
        dev.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T
        with pytest.raises(TetradHipError, match="tq_ls_add: tree 1") as info:
            dev.add_parents([trees[5], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8"):
            dev.add_parents(trees[5:9])
        dev.score_ranks(ranks[:1000])
        bad = np.array(quartets[:10], np.int32)
        bad[4, 1] = bad[4, 3]
        with pytest.raises(TetradHipError, match="tq_ls_score: quartet 4: repeated taxon"):
            dev.score(bad, counts=True)
        bad[4, 1] = T
        with pytest.raises(TetradHipError, match="quartet 4: taxon out of range"):
            dev.score(bad)
        with pytest.raises(TetradHipError, match="tq_ls_score_ranks: rank 1"):
            dev.score_ranks([5, comb(T, 4)])
        with pytest.raises(ValueError, match="exceeds"):
            dev.score_range(comb(T, 4) - 3, 4)
        with pytest.raises(TetradHipError, match="quartets have been scored"):
            dev.add_parents(trees[5:6])
        assert dev.ntrees == 5 and dev.nquartets == 1000
        sm.assert_matches(dev, None, *pairs_expected(5, 0, 1000), 5)
    for bad_T in (3, 1025):
        with pytest.raises(TetradHipError, match="tq_ls_create: T must be 4..1024"):
            LeafStability(bad_T, 4, engine=engine)
    for bad_n in (0, 8193):
        with pytest.raises(TetradHipError, match="max_trees must be 1..8192"):
            LeafStability(T, bad_n, engine=engine)


def test_replicate_loop_feeds_both_accumulators(engine):
    """bootstrap_trees(supertree="device", stability=acc, quartet_distances=acc2) on a source of the c1 shape (16 taxa,
    5 000 sites): both accumulators hold the returned trees, as adds made by hand do."""
    from tetrad_amd import synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.replicates import bootstrap_trees
    T, S, Q, nboots = 16, 5000, 1800, 8
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=synth.CONFIG_SEEDS["c1"], ambiguous=0.02)
    with LeafStability(T, nboots, engine=engine) as acc, QuartetDistances(T, nboots, engine=engine) as acc2:
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=5, workers=2, supertree="device",
                                stability=acc, quartet_distances=acc2)
        assert len(trees) == nboots == acc.ntrees == acc2.ntrees
        table = acc.score_all(counts=True)
        acc2.score_all()
        parents = [newick_to_parent(t)[0] for t in trees]
        with LeafStability(T, nboots) as hand, QuartetDistances(T, nboots) as hand2:
            hand.add_parents(parents)
            hand2.add_parents(parents)
            np.testing.assert_array_equal(hand.score_all(counts=True), table)
            hand2.score_all()
            assert_same(acc, hand)
            for a, b in zip(acc2.raw(), hand2.raw()):
                np.testing.assert_array_equal(a, b)
        w_counts, w_acc = sm.expected(parents, T, qm.all_quartets(T))
        sm.assert_matches(acc, table, w_counts, w_acc, nboots)
        assert sorted(acc.ranking().tolist()) == list(range(T)) and 0.0 <= acc.stability().min() <= acc.stability().max() <= 1.0
