"""GPU: the device execution of the quartet distance accumulator (`tq_qd_*` with a context: `tq_fit_table_kernel` at an
add; `tq_unrank_kernel`, `tq_qd_encode_kernel`, `tq_qd_gemm_kernel` per chunk of quartets; `tq_qd_final_kernel` at a read)
equals the host back end and the independent model of tests/qdist_model.py bit for bit -- across both table forms, the
tile boundaries and the k split of the product, the word and staged-chunk boundaries of the planes, quartet chunks,
repeated reads, clears, resets, streams, and in the replicate loop."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest

import consensus_model as cm
import qdist_model as qm
import treedist_model as dm
from tetrad_amd.qdist import QuartetDistances

pytestmark = pytest.mark.gpu

STAGED = 8 * 64             # quartets of one staged word chunk of the product


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def slices_used(nchunks, want):
    """The k slices of a product over `nchunks` staged word chunks when `want` are asked for: none is empty."""
    per = -(-nchunks // max(1, min(want, nchunks)))
    return -(-nchunks // per)


def assert_same(dev, host):
    for a, b in zip(dev.raw(), host.raw()):
        np.testing.assert_array_equal(a, b)
    assert dev.ntrees == host.ntrees and dev.nquartets == host.nquartets


@pytest.mark.parametrize("T", [4, 5, 33, 128, 129])
def test_device_equals_host_and_model(engine, T):
    """40 trees: one tile of the product with a tail of 24 empty rows; the table in LDS up to 128 taxa, through L2 above."""
    trees, quartets, ranks, *classes = qm.set_model(T, T)
    with QuartetDistances(T, 40, engine=engine) as dev, QuartetDistances(T, 40) as host:
        for acc in (dev, host):
            acc.add_parents(trees)
            qm.score_model(acc, quartets, ranks)
        qm.assert_matches(dev, classes, len(quartets))
        assert_same(dev, host)
        st = dev.stats()
        assert st["table_form"] == (1 if T <= 128 else 2) and st["tables"] == 40 and st["chunks"] == 1
        assert st["kslices"] == slices_used(-(-len(quartets) // STAGED), 4 * engine.device_info()["num_cu"])   # one tile pair


PAIRS_T, PAIRS_Q = 33, 5000


@lru_cache(maxsize=None)
def pairs_model():
    """65 independent random binary trees, each followed by one NNI of itself, over 5 000 sampled quartets: 79 plane
    words, 9 full staged word chunks and a tail of 7 words."""
    trees = dm.nni_pairs(PAIRS_T, 65, PAIRS_T)
    ranks = qm.sample_ranks(PAIRS_T, PAIRS_Q, PAIRS_T)
    quartets = qm.unrank(ranks, PAIRS_T)
    return (trees, quartets, ranks) + qm.expected(trees, PAIRS_T, quartets)


@pytest.mark.parametrize("N", [1, 2, 64, 65, 130])
def test_tile_boundaries_of_the_product(engine, N):
    """N = 130: three tiles per side, tile pairs off the diagonal (mirrored at the read), a tail of 2 rows."""
    trees, quartets, ranks, *classes = pairs_model()
    with QuartetDistances(PAIRS_T, N, engine=engine) as dev:
        dev.add_parents(trees[:N])
        dev.score_ranks(ranks)
        qm.assert_matches(dev, [c[:N, :N] for c in classes], PAIRS_Q)
        qm.assert_matches(dev, [c[:N, :N] for c in classes], PAIRS_Q)       # a second read mirrors again
        assert dev.stats()["chunk_words"] >= 79 and dev.stats()["chunks"] == 1


@pytest.mark.parametrize("Q", [1, 63, 64, 65, STAGED - 1, STAGED, STAGED + 1])
def test_word_and_staged_chunk_boundaries(engine, Q):
    """The last partial word and the last partial staged chunk."""
    trees, quartets, ranks, *_ = pairs_model()
    with QuartetDistances(PAIRS_T, 40, engine=engine) as dev:
        dev.add_parents(trees[:40])
        dev.score_ranks(ranks[:Q])
        qm.assert_matches(dev, qm.expected(trees[:40], PAIRS_T, quartets[:Q]), Q)


def test_deep_trees(engine):
    """1 024 taxa: a caterpillar (depths up to 1 023), a balanced and a random tree, tables read through L2."""
    T = 1024
    rng = np.random.default_rng(T)
    trees = [cm.caterpillar(T), cm.balanced(T), cm.random_binary(T, rng)]
    ranks = qm.sample_ranks(T, 2000, T)
    with QuartetDistances(T, 3, engine=engine) as dev, QuartetDistances(T, 3) as host:
        for acc in (dev, host):
            acc.add_parents(trees)
            acc.score_ranks(ranks)
        assert_same(dev, host)
        assert dev.stats()["table_form"] == 2
        assert (dev.resolved() == 2000).all() and dev.distance()[0, 1] > 0


@pytest.mark.parametrize("want", [1, 2, 7, 0])
def test_k_split_gives_identical_matrices(engine, want):
    """79 words are 10 staged chunks: 7 slices asked for take 2 chunks each, which makes 5; auto would like 4 workgroups
    per compute unit from 3 tile pairs and is capped by the 10 chunks."""
    trees, quartets, ranks, *classes = pairs_model()
    used = slices_used(10, want or -(-4 * engine.device_info()["num_cu"] // 3))
    assert used == {1: 1, 2: 2, 7: 5}.get(want, used)
    engine.set_option("qdist_kslices", want)
    try:
        with QuartetDistances(PAIRS_T, 65, engine=engine) as dev:
            dev.add_parents(trees[:65])
            dev.score_ranks(ranks)
            qm.assert_matches(dev, [c[:65, :65] for c in classes], PAIRS_Q)
            assert dev.stats()["kslices"] == used
    finally:
        engine.set_option("qdist_kslices", 0)


def test_quartet_chunks(engine):
    """A scratch budget of 100 000 bytes with room for 65 trees holds 24 plane words: 1 536 quartets, 4 chunks of 5 000."""
    trees, quartets, ranks, *classes = pairs_model()
    engine.set_option("qdist_scratch_bytes", 100_000)
    try:
        small = QuartetDistances(PAIRS_T, 65, engine=engine)
    finally:
        engine.set_option("qdist_scratch_bytes", 0)
    with small, QuartetDistances(PAIRS_T, 65, engine=engine) as one:
        for acc in (small, one):
            acc.add_parents(trees[:65])
            acc.score_ranks(ranks)
        qm.assert_matches(small, [c[:65, :65] for c in classes], PAIRS_Q)
        assert_same(small, one)
        assert small.stats()["chunk_quartets"] == 1536 and small.stats()["chunks"] == 4 and one.stats()["chunks"] == 1
        small.clear()
        small.score(quartets)                                       # the explicit array in chunks too
        assert small.stats()["chunks"] == 8
        assert_same(small, one)
        small.clear()
        small.score_range(100, 4000)                                # and a range
        one.clear()
        one.score_range(100, 4000)
        assert_same(small, one)
        qm.assert_matches(small, qm.expected(trees[:65], PAIRS_T, qm.all_quartets(PAIRS_T)[100:4100]), 4000)


def test_one_nni_and_one_contraction_over_all_quartets(engine):
    T = 33
    rng = np.random.default_rng(T)
    base = cm.unrooted(cm.random_binary(T, rng), T)
    moved = cm.nni(base, T, rng)
    sizes, side = qm.nni_parts(base, moved, T)
    n, Q = int(np.prod(sizes)), comb(T, 4)
    assert Q == 40920
    with QuartetDistances(T, 3, engine=engine) as dev:
        dev.add_parents([base, moved, qm.contract(base, T, side)])
        dev.score_all()
        A, B, C, D, E = dev.counts()
        assert B[0, 1] == n and C[0, 1] == D[0, 1] == E[0, 1] == 0 and A[0, 1] == Q - n
        assert C[0, 2] == n and B[0, 2] == D[0, 2] == E[0, 2] == 0
        assert dev.resolved().tolist() == [Q, Q, Q - n]


def test_stars_and_equal_trees(engine):
    T, Q = 33, comb(33, 4)
    tree = cm.random_binary(T, np.random.default_rng(7))
    with QuartetDistances(T, 80, engine=engine) as dev:
        dev.add_parents([cm.star(T)] * 3 + [tree])
        dev.score_all()
        A, B, C, D, E = dev.counts()
        assert dev.resolved().tolist() == [0, 0, 0, Q] and E[0, 1] == Q and D[0, 3] == Q and not A[:3].any()
        assert not B.any() and dev.distance()[0, 3] == Q
        dev.reset()
        dev.add_parents([tree] * 70)                                # every resolved bit equal: two tiles, all the same
        dev.score_all()
        same, both = dev.raw()
        assert (same == Q).all() and (both == Q).all() and not dev.distance().any()


def test_explicit_quartets_equal_their_ranks(engine):
    trees, quartets, ranks, *classes = pairs_model()
    rng = np.random.default_rng(2)
    shuffled = np.array([row[rng.permutation(4)] for row in quartets], np.int32)
    with QuartetDistances(PAIRS_T, 40, engine=engine) as dev:
        dev.add_parents(trees[:40])
        dev.score(shuffled)                                         # any order of the taxa
        qm.assert_matches(dev, [c[:40, :40] for c in classes], PAIRS_Q)


def test_streams_reads_between_scores_clear_and_reset(engine):
    import torch
    trees, quartets, ranks, *classes = pairs_model()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    N = 70
    want = [c[:N, :N] for c in classes]
    with QuartetDistances(PAIRS_T, N, engine=engine) as dev:
        dev.add_parents(trees[:30], stream=s1.cuda_stream)
        dev.add_parents(trees[30:N], stream=s2.cuda_stream)
        for i, lo in enumerate(range(0, PAIRS_Q, 700)):             # scores alternating between two streams
            dev.score_ranks(ranks[lo:lo + 700], stream=(s1, s2)[i % 2].cuda_stream)
        qm.assert_matches(dev, want, PAIRS_Q)
        dev.clear()                                                 # keeps the trees
        assert dev.ntrees == N and dev.nquartets == 0 and not dev.raw()[0].any() and not dev.raw()[1].any()
        dev.score_ranks(ranks[:2000])
        qm.assert_matches(dev, qm.expected(trees[:N], PAIRS_T, quartets[:2000]), 2000)      # score, read,
        dev.score_ranks(ranks[2000:])
        qm.assert_matches(dev, want, PAIRS_Q)                       # score, read
        dev.reset()
        assert dev.ntrees == 0 and dev.raw()[0].shape == (0, 0)
        dev.score_ranks(ranks)                                      # no trees: a no-op
        assert dev.nquartets == 0
        dev.add_parents(trees[33:39])                               # a smaller set: another row pitch, nothing stale
        dev.score_ranks(ranks)
        qm.assert_matches(dev, [c[33:39, 33:39] for c in classes], PAIRS_Q)
    torch.cuda.synchronize()


def test_refusals_leave_the_device_state_unchanged(engine):
    from tetrad_amd._lib import TetradHipError
    T = PAIRS_T
    trees, quartets, ranks, *classes = pairs_model()
    with QuartetDistances(T, 8, engine=engine) as dev:
        dev.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T
        with pytest.raises(TetradHipError, match="tq_qd_add: tree 1") as info:
            dev.add_parents([trees[5], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8"):
            dev.add_parents(trees[5:9])
        dev.score_ranks(ranks[:1000])
        bad = np.array(quartets[:10], np.int32)
        bad[4, 1] = bad[4, 3]
        with pytest.raises(TetradHipError, match="quartet 4: repeated taxon"):
            dev.score(bad)
        bad[4, 1] = T
        with pytest.raises(TetradHipError, match="quartet 4: taxon out of range"):
            dev.score(bad)
        with pytest.raises(TetradHipError, match="rank 1"):
            dev.score_ranks([5, comb(T, 4)])
        with pytest.raises(TetradHipError, match="quartets have been scored"):
            dev.add_parents(trees[5:6])
        assert dev.ntrees == 5 and dev.nquartets == 1000
        qm.assert_matches(dev, qm.expected(trees[:5], T, quartets[:1000]), 1000)
    for bad_T in (3, 1025):
        with pytest.raises(TetradHipError, match="T must be 4..1024"):
            QuartetDistances(bad_T, 4, engine=engine)
    for bad_n in (0, 8193):
        with pytest.raises(TetradHipError, match="max_trees must be 1..8192"):
            QuartetDistances(T, bad_n, engine=engine)


def test_replicate_loop_feeds_both_accumulators(engine):
    """bootstrap_trees(supertree="device", quartet_distances=acc, distances=acc2) on a source of the c1 shape (16 taxa,
    5 000 sites): both accumulators hold the returned trees, as adds made by hand do."""
    from tetrad_amd import synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.replicates import bootstrap_trees
    from tetrad_amd.treedist import TreeDistances
    T, S, Q, nboots = 16, 5000, 1800, 8
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=synth.CONFIG_SEEDS["c1"], ambiguous=0.02)
    with QuartetDistances(T, nboots, engine=engine) as acc, TreeDistances(T, nboots, engine=engine) as acc2:
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=5, workers=2, supertree="device",
                                quartet_distances=acc, distances=acc2)
        assert len(trees) == nboots == acc.ntrees == acc2.ntrees
        acc.score_all()
        parents = [newick_to_parent(t)[0] for t in trees]
        with QuartetDistances(T, nboots) as hand, TreeDistances(T, nboots) as hand2:
            hand.add_parents(parents)
            hand.score_all()
            hand2.add_parents(parents)
            assert_same(acc, hand)
            for a, b in zip(acc2.raw(), hand2.raw()):
                np.testing.assert_array_equal(a, b)
        qm.assert_matches(acc, qm.expected(parents, T, qm.all_quartets(T)), comb(T, 4))
        index, total = acc.medoid()
        assert 0 <= index < nboots and total == int(acc.distance()[index].sum())
        assert 0.0 <= acc.mean_distance() <= comb(T, 4) and acc.normalized().max() <= 1.0
