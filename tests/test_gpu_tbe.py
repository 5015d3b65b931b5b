"""GPU: the device execution of the transfer bootstrap accumulator (`tq_tbe_*` with a context: `tq_cons_mask_kernel`
followed by `tq_tbe_kernel`) equals the host back end and the independent model of tests/tbe_model.py bit for bit, in
`raw()` and in the per-tree matrix -- across the word, word-chunk and tile boundaries, stale scratch, chunk counts,
streams, one hot counter, and in the replicate loop."""
import numpy as np
import pytest

import consensus_model as cm
import tbe_model as tm
from concordance_split_model import collapse_clade
from tetrad_amd.consensus import Consensus
from tetrad_amd.tbe import TransferSupport

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


# reference 0: a random rooted tree; 32: the caterpillar ((((0,1),2),3),...), whose canonical masks (without taxon 0) are
# the heavy side for half of its branches, so that delta comes from T - d; 24: a tree with a polytomy
@pytest.mark.parametrize("T", [4, 5, 33, 64, 65, 129])
def test_device_equals_host_and_model(engine, T):
    for ref in (0, 32, 24):
        trees, masks, p, phi = tm.set_model(T, T, ref)
        with TransferSupport(T, trees[ref], engine=engine) as dev, TransferSupport(T, trees[ref]) as host:
            got = dev.add_parents(trees, per_tree=True)
            want = host.add_parents(trees, per_tree=True)
            tm.assert_matches(dev, masks, p, phi)
            np.testing.assert_array_equal(got, phi)
            np.testing.assert_array_equal(got, want)
            assert_same(dev, host)
            assert dev.stats()["chunks"] == 1
            if ref == 32 and T >= 5:
                assert (masks.sum(axis=1) > T // 2).any() and (masks.sum(axis=1) + p == T)[masks.sum(axis=1) > T // 2].all()
            dev.reset()
            dev.add_parents(trees)                                 # without the matrix: the same sums
            assert_same(dev, host)


@pytest.mark.parametrize("T", [1025, 4096])
def test_large_trees(engine, T):
    """W = 17 crosses the word chunk of 8 twice and ends in a chunk of one word; E and M exceed one tile of either
    operand.  W = 64 is the limit.  All entries against the host; 16 seeded (branch, tree) pairs against the model."""
    rng = np.random.default_rng(T)
    rand = cm.random_binary(T, rng)
    reps = [cm.balanced(T), rand, cm.caterpillar(T), collapse_clade(rand, T, 0.3)]
    ref = cm.random_binary(T, rng)
    with TransferSupport(T, ref, engine=engine) as dev, TransferSupport(T, ref) as host:
        got = dev.add_parents(reps, per_tree=True)
        want = host.add_parents(reps, per_tree=True)
        np.testing.assert_array_equal(got, want)
        assert_same(dev, host)
        masks, p, _ = dev.raw()
        assert len(p) == T - 3 and (got <= p - 1).all() and got.max() > 1
        pairs = list(zip(rng.integers(0, T - 3, 16).tolist(), rng.integers(0, len(reps), 16).tolist()))
        for r in sorted({r for _, r in pairs}):
            mine = [e for e, rr in pairs if rr == r]
            side = {e: frozenset(np.flatnonzero(masks[e]).tolist()) for e in mine}
            best = {e: T for e in mine}
            for s in tm.each_edge_side(reps[r], T):                # one walk per tree: every edge, tip edges included
                for e in mine:
                    best[e] = min(best[e], tm.delta(side[e], s, T))
            assert [int(got[r, e]) for e in mine] == [best[e] for e in mine], r
    if T == 1025:                                                  # the heavy-side masks of a caterpillar reference
        with TransferSupport(T, cm.caterpillar(T), engine=engine) as dev, TransferSupport(T, cm.caterpillar(T)) as host:
            np.testing.assert_array_equal(dev.add_parents(reps, per_tree=True), host.add_parents(reps, per_tree=True))
            assert_same(dev, host)


@pytest.mark.parametrize("T", [65, 129])
def test_stale_scratch_beyond_the_nodes_of_a_tree(engine, T):
    """A star (M = 1) and a polytomy after binary trees: their scratch slots still hold the earlier trees' masks in the
    rows v >= M -- among them every branch of the reference, which would give phi = 0."""
    trees, masks, p, phi = tm.set_model(T, T, 0)
    binary = [trees[0], trees[1], trees[2], trees[3]]
    late = [trees[36], trees[24], trees[36], trees[25]]            # star, polytomy, star, polytomy
    with TransferSupport(T, trees[0], engine=engine) as dev:
        dev.add_parents(binary)
        got = dev.add_parents(late, per_tree=True)
        np.testing.assert_array_equal(got, phi[[36, 24, 36, 25]])
        np.testing.assert_array_equal(got[0], p - 1)
        tm.assert_matches(dev, masks, p, phi[[0, 1, 2, 3, 36, 24, 36, 25]])


def test_chunks_streams_and_reset(engine):
    """A scratch budget of 80 000 bytes holds about 12 trees of 129 taxa: 40 trees take 4 chunks, the default one."""
    import torch
    T = 129
    trees, masks, p, phi = tm.set_model(T, T, 0)
    engine.set_option("cons_scratch_bytes", 80_000)
    try:
        small = TransferSupport(T, trees[0], engine=engine)
    finally:
        engine.set_option("cons_scratch_bytes", 0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with small, TransferSupport(T, trees[0], engine=engine) as one:
        got = small.add_parents(trees, per_tree=True)
        one.add_parents(trees)
        st = small.stats()
        assert st["chunk_trees"] * 3 <= len(trees) and st["chunks"] == -(-len(trees) // st["chunk_trees"]) >= 4
        assert one.stats()["chunks"] == 1
        np.testing.assert_array_equal(got, phi)
        tm.assert_matches(small, masks, p, phi)
        assert_same(small, one)
        for acc in (small, one):
            for rep in range(2):
                acc.reset()
                assert acc.ntrees == 0 and not acc.raw()[2].any()
                for i in range(0, len(trees), 6):                  # adds alternating between two streams
                    acc.add_parents(trees[i:i + 6], stream=(s1, s2)[(i // 6) % 2].cuda_stream)
                tm.assert_matches(acc, masks, p, phi)
    torch.cuda.synchronize()


def test_a_star_reference_has_no_branches(engine):
    T = 33
    trees = cm.tree_set(T, T)
    with TransferSupport(T, cm.star(T), engine=engine) as dev:
        got = dev.add_parents(trees, per_tree=True)
        masks, p, phi_sum = dev.raw()
        assert got.shape == (40, 0) and masks.shape == (0, T) and len(p) == len(phi_sum) == 0 and dev.ntrees == 40
        assert dev.supports().shape == (0,) and dev.map_supports() == "(" + ",".join(str(t) for t in range(T)) + ");"


def test_one_hot_branch(engine):
    """T = 4: one branch, and every one of 10 000 replicates adds its phi to the same word."""
    T, R = 4, 10_000
    ref = cm.balanced(T)                                           # ((0,1),(2,3))
    other = np.array([4, 5, 4, 5, 6, 6, -1], np.int32)             # ((0,2),(1,3))
    kinds = [ref, other, cm.star(T), cm.unrooted(ref, T)]
    pick = np.random.default_rng(4).integers(0, 4, R)
    want = np.array([0, 1, 1, 0])[pick]
    with TransferSupport(T, ref, engine=engine) as dev, TransferSupport(T, ref) as host:
        got = dev.add_parents([kinds[k] for k in pick], per_tree=True)
        host.add_parents([kinds[k] for k in pick])
        np.testing.assert_array_equal(got[:, 0], want)
        assert dev.raw()[2].tolist() == [int(want.sum())] and dev.raw()[1].tolist() == [2]
        assert_same(dev, host)
        dev.add_parents([kinds[k] for k in pick])
        assert dev.raw()[2].tolist() == [2 * int(want.sum())] and dev.ntrees == 2 * R


def test_refusals_leave_the_device_sums_unchanged(engine):
    from tetrad_amd._lib import TetradHipError
    T = 33
    trees, masks, p, phi = tm.set_model(T, T, 0)
    with TransferSupport(T, trees[0], engine=engine) as dev:
        dev.add_parents(trees[:5])
        cyc = np.array(trees[1], np.int32)
        cyc[T], cyc[T + 1] = T + 1, T
        with pytest.raises(TetradHipError, match="tq_tbe_add: tree 1") as info:
            dev.add_parents([trees[5], cyc], per_tree=True)
        assert info.value.code == -1
        tm.assert_matches(dev, masks, p, phi[:5])
    for bad_T in (3, 4097):
        with pytest.raises(TetradHipError, match="T must be 4..4096"):
            TransferSupport(bad_T, cm.star(bad_T), engine=engine)


def test_replicate_loop_feeds_both_accumulators(engine):
    """bootstrap_trees(supertree="device", transfer=acc, consensus=acc2) on a source of the c1 shape (16 taxa, 5 000
    sites): both accumulators hold the returned trees, as adds made by hand do."""
    from tetrad_amd import synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.replicates import bootstrap_trees
    T, S, Q, nboots = 16, 5000, 1800, 8
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=synth.CONFIG_SEEDS["c1"], ambiguous=0.02)
    ref = cm.balanced(T)
    with TransferSupport(T, ref, engine=engine) as acc, Consensus(T, engine=engine) as acc2:
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=5, workers=2, supertree="device",
                                transfer=acc, consensus=acc2)
        assert len(trees) == nboots == acc.ntrees == acc2.ntrees
        parents = [newick_to_parent(t)[0] for t in trees]
        with TransferSupport(T, ref) as hand, Consensus(T) as hand2:
            hand.add_parents(parents)
            hand2.add_parents(parents)
            assert_same(acc, hand)
            for a, b in zip(acc2.raw(), hand2.raw()):
                np.testing.assert_array_equal(a, b)
        masks, p, want = tm.expected(ref, parents, T)
        tm.assert_matches(acc, masks, p, want)
        assert all(0 <= x <= 100 for x in acc.percents())
