"""GPU: the device execution of the consensus accumulator (`tq_cons_*` with a context: mask, insert, count and gather
kernels) equals the independent model of tests/consensus_model.py and the host back end bit for bit -- across word and
size boundaries, chunk counts, hash widths (the collision path), streams, the split limit, and in the replicate loop."""
import re

import numpy as np
import pytest

import consensus_model as cm
from concordance_split_model import collapse_clade
from tetrad_amd.consensus import Consensus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def set65():
    """The T = 65 set with its model and host table, shared by the tests that vary how the device gets there."""
    T = 65
    trees = cm.tree_set(T, seed=T)
    tab, n = cm.model_of(trees, T)
    with Consensus(T) as host:
        host.add_parents(trees)
        cm.assert_matches(host, tab, n, T)
        raw = host.raw()
        nwk = [host.tree(f) for f in (0.5, 0.2)]
    return T, trees, tab, n, raw, nwk


def assert_equals_host(dev, raw, nwk=None):
    got = dev.raw()
    np.testing.assert_array_equal(got[1], raw[1])
    np.testing.assert_array_equal(got[0], raw[0])
    assert got[2] == raw[2]
    if nwk is not None:
        assert [dev.tree(f) for f in (0.5, 0.2)] == nwk


@pytest.mark.parametrize("T", [5, 33, 64, 65, 129, 1025])
def test_device_equals_model_and_host(engine, T):
    trees = cm.tree_set(T, seed=T)
    tab, n = cm.model_of(trees, T)
    with Consensus(T, engine=engine) as dev, Consensus(T) as host:
        dev.add_parents(trees)
        host.add_parents(trees)
        cm.assert_matches(dev, tab, n, T)
        assert_equals_host(dev, host.raw())
        for f in (0.5, 0.2):
            k = cm.min_count(f, n)
            assert dev.tree(f) == host.tree(f) == cm.consensus(tab, T, n, k)
        given = trees[3]
        cd, md = dev.support_of(given)
        ch, mh = host.support_of(given)
        np.testing.assert_array_equal(cd, ch)
        np.testing.assert_array_equal(md, mh)
        st = dev.stats()
        assert st["chunks"] == 1 and st["unresolved"] == 0 and st["device_entries"] == len(tab)


def test_device_at_the_taxon_limit(engine):
    """T = 4096: balanced, random, a caterpillar (4 093 heights of one node each) and a polytomy of about 0.3 T tips."""
    T = 4096
    rng = np.random.default_rng(40)
    rand = cm.random_binary(T, rng)
    trees = [cm.balanced(T), rand, cm.caterpillar(T), collapse_clade(rand, T, 0.3)]
    tab, n = cm.model_of(trees, T)
    with Consensus(T, engine=engine) as dev, Consensus(T) as host:
        dev.add_parents(trees)
        host.add_parents(trees)
        cm.assert_matches(dev, tab, n, T)
        assert_equals_host(dev, host.raw())
        assert dev.tree(0.5) == host.tree(0.5) == "(" + ",".join(str(t) for t in range(T)) + ");"
        assert dev.tree_min_count(2) == host.tree_min_count(2) == cm.consensus(tab, T, n, 2)
        assert dev.stats()["unresolved"] == 0


def test_chunks(engine):
    """a scratch budget of 80 000 bytes holds 12 trees of 129 taxa: 40 trees take 4 chunks; the default takes one"""
    T = 129
    trees = cm.tree_set(T, seed=7)
    tab, n = cm.model_of(trees, T)
    engine.set_option("cons_scratch_bytes", 80_000)
    try:
        small = Consensus(T, engine=engine)
    finally:
        engine.set_option("cons_scratch_bytes", 0)
    with small, Consensus(T, engine=engine) as one:
        small.add_parents(trees)
        one.add_parents(trees)
        st = small.stats()
        assert st["chunk_trees"] * 3 <= len(trees) and st["chunks"] >= 3
        assert st["chunks"] == -(-len(trees) // st["chunk_trees"])
        assert one.stats()["chunks"] == 1
        cm.assert_matches(small, tab, n, T)
        assert_equals_host(small, one.raw(), [one.tree(f) for f in (0.5, 0.2)])
        small.add_parents(trees[:5])                               # a second add, again in chunks of its own
        one.add_parents(trees[:5])
        assert_equals_host(small, one.raw())


@pytest.mark.parametrize("bits", [64, 12, 4])
def test_hash_width_does_not_change_the_result(engine, set65, bits):
    T, trees, tab, n, raw, nwk = set65
    engine.set_option("cons_hash_bits", bits)
    try:
        dev = Consensus(T, engine=engine)
    finally:
        engine.set_option("cons_hash_bits", 0)
    with dev:
        dev.add_parents(trees[:25])
        dev.add_parents(trees[25:])
        cm.assert_matches(dev, tab, n, T)
        assert_equals_host(dev, raw, nwk)
        st = dev.stats()
        total = int(raw[1].sum())
        assert st["hash_bits"] == bits and st["device_entries"] + st["host_entries"] == len(tab)
        if bits == 64:
            assert st["unresolved"] == 0 and st["host_entries"] == 0
        if bits == 4:                                              # 16 keys: at most 16 splits have an entry on the device
            assert st["device_entries"] <= 16 and 2 * st["unresolved"] > total, st


def test_two_streams_and_reset(engine, set65):
    import torch
    T, trees, tab, n, raw, nwk = set65
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with Consensus(T, engine=engine) as dev:
        for rep in range(2):
            for i in range(0, len(trees), 6):
                s = (s1, s2)[(i // 6) % 2]
                dev.add_parents(trees[i:i + 6], stream=s.cuda_stream)
            assert_equals_host(dev, raw, nwk)
            dev.reset()
            assert dev.ntrees == 0 and len(dev.raw()[1]) == 0
    torch.cuda.synchronize()


def test_split_limit_is_an_error_and_the_context_stays_usable(engine, set65):
    from tetrad_amd import synth
    from tetrad_amd._lib import TetradHipError
    T, trees, tab, n, raw, nwk = set65
    tmparr, tmpmap = synth.simulate_tmparr(10, 1500, seed=3)
    quartets = synth.all_quartets(10)[:32]
    engine.set_data(tmparr, tmpmap)
    before = engine.resolve(quartets, True)
    with Consensus(T, max_splits=len(tab), engine=engine) as dev:
        dev.add_parents(trees)
        assert_equals_host(dev, raw, nwk)
    with Consensus(T, max_splits=len(tab) - 1, engine=engine) as dev:
        with pytest.raises(TetradHipError, match="max_splits") as info:
            dev.add_parents(trees)
            dev.raw()
        assert info.value.code == -1
        with pytest.raises(TetradHipError, match="max_splits"):
            dev.tree()
        after = engine.resolve(quartets, True)
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)
        dev.reset()
        dev.add_parents(trees[:8])
        cm.assert_matches(dev, *cm.model_of(trees[:8], T), T)


def test_replicate_loop_feeds_the_accumulator(engine):
    """bootstrap_trees(supertree="device", consensus=acc): the accumulator holds the returned trees.  T = 16 has 1 820
    quartets in all; every replicate samples 1 800 of them."""
    from tetrad_amd import synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.replicates import bootstrap_trees
    T, S, Q, nboots = 16, 4000, 1800, 8
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=12, ambiguous=0.02)
    with Consensus(T, engine=engine) as acc:
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=5, workers=2, supertree="device",
                                consensus=acc)
        assert len(trees) == nboots == acc.ntrees
        tab, n = cm.model_of([newick_to_parent(t)[0] for t in trees], T)
        cm.assert_matches(acc, tab, n, T)
        nwk = acc.tree()
        assert nwk == cm.consensus(tab, T, n, cm.min_count(0.5, n))
        supports = [int(x) for x in re.findall(r"\)(\d+)", nwk)]
        assert supports and all(50 < x <= 100 for x in supports)
        mapped = acc.map_supports(trees[0])
        assert all(0 <= int(x) <= 100 for x in re.findall(r"\)(\d+)", mapped))
