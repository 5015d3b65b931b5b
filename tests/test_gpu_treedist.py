"""GPU: the device execution of the tree distance accumulator (`tq_rf_*` with a context: the consensus mask and insert
kernels, `tq_rf_ident_kernel`, then per read `tq_rf_scatter_kernel`, `tq_rf_gemm_kernel`, `tq_rf_final_kernel`) equals
the host back end and the independent model of tests/treedist_model.py bit for bit -- across the word boundaries of the
masks, the tile and word-chunk boundaries of the product, tree chunks, column chunks, hash widths, repeated reads,
resets, streams, and in the replicate loop."""
from functools import lru_cache

import numpy as np
import pytest

import consensus_model as cm
import treedist_model as dm
from concordance_split_model import collapse_clade
from tetrad_amd.consensus import Consensus
from tetrad_amd.treedist import TreeDistances

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def assert_same(dev, host):
    for a, b in zip(dev.raw(), host.raw()):
        np.testing.assert_array_equal(a, b)
    assert dev.ntrees == host.ntrees


@pytest.mark.parametrize("T", [4, 5, 33, 64, 65, 129])
def test_device_equals_host_and_model(engine, T):
    """40 trees: one tile of the product with a tail of 24 empty rows."""
    trees, nsplits, shared, rf, columns = dm.set_model(T, T)
    with TreeDistances(T, 40, engine=engine) as dev, TreeDistances(T, 40) as host:
        dev.add_parents(trees)
        host.add_parents(trees)
        dm.assert_matches(dev, nsplits, shared, rf)
        assert_same(dev, host)
        st = dev.stats()
        assert st["columns"] == columns == host.stats()["columns"] and st["chunks"] == 1
        assert st["col_chunks"] == (1 if columns else 0)
        assert dev.ndistinct == host.ndistinct


PAIRS_T, PAIRS_SEED = 33, 33


@lru_cache(maxsize=None)
def pairs_model():
    trees = dm.nni_pairs(PAIRS_T, 65, PAIRS_SEED)
    return (trees,) + dm.expected(trees, PAIRS_T)


@pytest.mark.parametrize("N", [1, 2, 64, 65, 130])
def test_tile_boundaries_of_the_product(engine, N):
    """65 independent random binary trees, each followed by one NNI of itself.  N = 130: three tiles per side, tile
    pairs off the diagonal, a tail of 2 rows; at least 1 025 columns make 17 words: two full word chunks and a tail."""
    T = PAIRS_T
    trees, nsplits, shared, rf, columns = pairs_model()
    want_columns = columns if N == 130 else dm.expected(trees[:N], T)[3]
    with TreeDistances(T, N, engine=engine) as dev, TreeDistances(T, N) as host:
        dev.add_parents(trees[:N])
        host.add_parents(trees[:N])
        dm.assert_matches(dev, nsplits[:N], shared[:N, :N], rf[:N, :N])
        assert_same(dev, host)
        assert dev.stats()["columns"] == want_columns
        if N == 130:
            assert want_columns >= 1025
            assert dev.stats()["col_chunks"] == 1
        if N == 1:
            assert want_columns == 0 and dev.stats()["col_chunks"] == 0


def test_all_trees_equal(engine):
    """Every bit of the bit rows is set: rf all zero, shared all nsplits."""
    T, N = 33, 70
    tree = cm.random_binary(T, np.random.default_rng(7))
    with TreeDistances(T, N, engine=engine) as dev:
        dev.add_parents([tree] * N)
        assert (dev.nsplits() == T - 3).all() and (dev.shared() == T - 3).all() and not dev.rf().any()
        assert dev.stats()["columns"] == T - 3 == dev.ndistinct


@pytest.mark.parametrize("N", [1, 3, 70])
def test_all_stars(engine, N):
    """No split, no column: nothing is multiplied, the matrices are zero."""
    T = 33
    with TreeDistances(T, 80, engine=engine) as dev:
        dev.add_parents([cm.star(T)] * N)
        n, s, d = dev.raw()
        assert n.shape == (N,) and s.shape == d.shape == (N, N) and not n.any() and not s.any() and not d.any()
        st = dev.stats()
        assert st["columns"] == 0 and st["col_chunks"] == 0 and dev.ndistinct == 0


def test_unrelated_trees_have_no_column_when_they_share_nothing(engine):
    """Two trees without a common split: C = 0 although both have splits."""
    T = 6
    a = np.array([6, 6, 7, 7, 8, 8, 9, 9, 9, -1], np.int32)        # ((0,1),(2,3),(4,5))
    b = np.array([6, 7, 6, 8, 7, 8, 9, 9, 9, -1], np.int32)        # ((0,2),(1,4),(3,5))
    with TreeDistances(T, 2, engine=engine) as dev:
        dev.add_parents([a, b])
        assert dev.nsplits().tolist() == [3, 3] and dev.rf().tolist() == [[0, 6], [6, 0]]
        assert dev.shared().tolist() == [[3, 0], [0, 3]]
        assert dev.stats()["columns"] == 0 and dev.stats()["col_chunks"] == 0 and dev.ndistinct == 6


def large_trees(T):
    rng = np.random.default_rng(T)
    rand = cm.unrooted(cm.random_binary(T, rng), T)
    return [cm.balanced(T), rand, cm.caterpillar(T), collapse_clade(rand, T, 0.3), cm.nni(rand, T, rng)]


@pytest.mark.parametrize("T", [1025, 4096])
def test_large_trees(engine, T):
    """W = 17 crosses the lane group of 32; W = 64 is the limit.  Balanced, random, caterpillar, the random tree with a
    clade collapsed, and one NNI of the random tree."""
    trees = large_trees(T)
    with TreeDistances(T, 5, engine=engine) as dev, TreeDistances(T, 5) as host:
        dev.add_parents(trees)
        host.add_parents(trees)
        assert_same(dev, host)
        n, s, d = dev.nsplits(), dev.shared(), dev.rf()
        assert d[1, 4] == 2 and s[1, 4] == T - 4
        assert not np.diag(d).any() and (d == d.T).all() and (s == s.T).all() and (np.diag(s) == n).all()
        assert n[[0, 1, 2, 4]].tolist() == [T - 3] * 4 and 0 < n[3] < T - 3
        assert s[1, 3] == n[3] and d[1, 3] == T - 3 - n[3]         # collapsing only removes splits
        if T == 1025:
            want = dm.expected(trees, T)
            dm.assert_matches(dev, *want[:3])
            assert dev.stats()["columns"] == want[3]


def test_tree_chunks_and_column_chunks(engine):
    """A scratch budget of 80 000 bytes holds about 10 trees of 129 taxa, and with room for 4 096 trees 2 words of bit
    row per tree: 40 trees take 4 tree chunks and the columns at least 3 chunks of 128."""
    T = 129
    trees, nsplits, shared, rf, columns = dm.set_model(T, T)
    assert columns > 2 * 128
    engine.set_option("cons_scratch_bytes", 80_000)
    try:
        small = TreeDistances(T, 4096, engine=engine)
    finally:
        engine.set_option("cons_scratch_bytes", 0)
    with small, TreeDistances(T, 4096, engine=engine) as one:
        small.add_parents(trees)
        one.add_parents(trees)
        dm.assert_matches(small, nsplits, shared, rf)
        dm.assert_matches(one, nsplits, shared, rf)
        assert_same(small, one)
        st = small.stats()
        assert st["chunk_trees"] * 3 < len(trees) and st["chunks"] == -(-len(trees) // st["chunk_trees"]) >= 4
        assert st["col_words_chunk"] == 2 and st["col_chunks"] == -(-columns // 128) >= 3 and st["columns"] == columns
        st = one.stats()
        assert st["chunks"] == 1 and st["col_chunks"] == 1 and st["columns"] == columns


def test_hash_widths_give_identical_matrices(engine):
    """With 4 hash bits nearly every split loses its collision and gets its id from the host map; with 12 some do."""
    T = 65
    trees, nsplits, shared, rf, columns = dm.set_model(T, T)
    unresolved = {}
    for bits in (64, 12, 4):
        engine.set_option("cons_hash_bits", bits)
        try:
            dev = TreeDistances(T, 40, engine=engine)
        finally:
            engine.set_option("cons_hash_bits", 0)
        with dev:
            dev.add_parents(trees[:25])
            dev.add_parents(trees[25:])
            dm.assert_matches(dev, nsplits, shared, rf)
            st = dev.stats()
            assert st["hash_bits"] == bits and st["columns"] == columns
            unresolved[bits] = st["unresolved"]
            assert st["dev_entries"] <= (16 if bits == 4 else 10 ** 9)
    assert unresolved[64] == 0 and unresolved[4] > int(nsplits.sum()) // 2


def test_reads_between_adds_reset_and_streams(engine):
    import torch
    T = 65
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with TreeDistances(T, 40, engine=engine) as dev:
        dev.add_parents(trees[:20])
        dm.assert_matches(dev, nsplits[:20], shared[:20, :20], rf[:20, :20])
        dm.assert_matches(dev, nsplits[:20], shared[:20, :20], rf[:20, :20])   # a second read of the same state
        dev.add_parents(trees[20:])
        dm.assert_matches(dev, nsplits, shared, rf)                 # shared is zeroed at every finalise
        dev.reset()
        assert dev.ntrees == 0 and dev.rf().shape == (0, 0)
        dev.add_parents(trees[33:39])                               # a smaller set: no stale ids, no stale bit rows
        dm.assert_matches(dev, nsplits[33:39], shared[33:39, 33:39], rf[33:39, 33:39])
        assert dev.stats()["columns"] == dm.expected(trees[33:39], T)[3]
        dev.reset()
        for i in range(0, len(trees), 6):                          # adds alternating between two streams
            dev.add_parents(trees[i:i + 6], stream=(s1, s2)[(i // 6) % 2].cuda_stream)
        dm.assert_matches(dev, nsplits, shared, rf)
    torch.cuda.synchronize()


def test_refusals_leave_the_device_state_unchanged(engine):
    from tetrad_amd._lib import TetradHipError
    T = 33
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    with TreeDistances(T, 8, engine=engine) as dev:
        dev.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T
        with pytest.raises(TetradHipError, match="tq_rf_add: tree 1") as info:
            dev.add_parents([trees[5], cyc])
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_trees = 8"):
            dev.add_parents(trees[5:9])
        assert dev.ntrees == 5
        dm.assert_matches(dev, nsplits[:5], shared[:5, :5], rf[:5, :5])
    for bad_T in (3, 4097):
        with pytest.raises(TetradHipError, match="T must be 4..4096"):
            TreeDistances(bad_T, 4, engine=engine)


@pytest.mark.parametrize("bits", [64, 4])
def test_more_distinct_splits_than_max_splits_is_refused_until_a_reset(engine, bits):
    """As the host back end (tests/test_treedist_cpu.py): the add that crosses max_splits fails -- a device add when its
    chunk is drained, here by the read behind it --, every later call fails, a reset makes the accumulator usable.  With
    64 hash bits the device table itself runs full.  With 4 it holds at most 16 of the 59 splits, the others get
    their ids from the host map, and that map runs full while the drain walks the chunk's unresolved masks."""
    from tetrad_amd._lib import TetradHipError
    T = 33
    trees, nsplits, shared, rf, _ = dm.set_model(T, T)
    two = np.ix_([0, 28], [0, 28])
    distinct = len(dm.splits(trees[0], T) | dm.splits(trees[28], T))
    assert distinct > 16 and dm.splits(trees[32], T) - dm.splits(trees[0], T) - dm.splits(trees[28], T)
    engine.set_option("cons_hash_bits", bits)
    try:
        with TreeDistances(T, 8, max_splits=distinct, engine=engine) as dev:
            dev.add_parents([trees[0], trees[28]])
            dm.assert_matches(dev, nsplits[[0, 28]], shared[two], rf[two])
            assert dev.ndistinct == distinct
            with pytest.raises(TetradHipError, match="more than max_splits = %d distinct splits" % distinct) as info:
                dev.add_parents([trees[32]])                        # brings new splits
                dev.rf()
            assert info.value.code == -1
            with pytest.raises(TetradHipError, match="reset the accumulator"):
                dev.rf()
            with pytest.raises(TetradHipError, match="reset the accumulator"):
                dev.add_parents([trees[0]])
            st = dev.stats()
            assert st["hash_bits"] == bits and (bits == 64 or st["dev_entries"] <= 16)
            dev.reset()
            dev.add_parents([trees[0], trees[28]])
            dm.assert_matches(dev, nsplits[[0, 28]], shared[two], rf[two])
            assert dev.stats()["hash_bits"] == bits
    finally:
        engine.set_option("cons_hash_bits", 0)


def test_replicate_loop_feeds_both_accumulators(engine):
    """bootstrap_trees(supertree="device", distances=acc, consensus=acc2) on a source of the c1 shape (16 taxa, 5 000
    sites): both accumulators hold the returned trees, as adds made by hand do."""
    from tetrad_amd import synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.replicates import bootstrap_trees
    T, S, Q, nboots = 16, 5000, 1800, 8
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=synth.CONFIG_SEEDS["c1"], ambiguous=0.02)
    with TreeDistances(T, nboots, engine=engine) as acc, Consensus(T, engine=engine) as acc2:
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=5, workers=2, supertree="device",
                                distances=acc, consensus=acc2)
        assert len(trees) == nboots == acc.ntrees == acc2.ntrees
        parents = [newick_to_parent(t)[0] for t in trees]
        with TreeDistances(T, nboots) as hand, Consensus(T) as hand2:
            hand.add_parents(parents)
            hand2.add_parents(parents)
            assert_same(acc, hand)
            for a, b in zip(acc2.raw(), hand2.raw()):
                np.testing.assert_array_equal(a, b)
        dm.assert_matches(acc, *dm.expected(parents, T)[:3])
        index, total = acc.medoid()
        assert 0 <= index < nboots and total == int(acc.rf()[index].sum()) and 0.0 <= acc.mean_rf() <= 2 * (T - 3)
