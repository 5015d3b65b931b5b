"""GPU: the taxon counts of the resident replicate.  The standard is device = host execution =
the independent model of tests/taxdist_model.py, bit for bit, on all four slots."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import taxdist_model as tm

pytestmark = pytest.mark.gpu

GOLDENS = ["tiny_T5_S37", "one_site_T5_S1", "edge_T7_S130", "sparse_T10_S257", "dense_T8_S400", "carry_T6_S2500"]


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def random_matrix(T, S, seed, missing=0.3):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, size=(T, S), dtype=np.uint8)
    a[rng.random((T, S)) < missing] = 78
    return a, np.arange(S, dtype=np.uint32)


def assert_three_agree(engine, tmparr, starts=None):
    from tetrad_amd import distance
    got = engine.taxon_counts(starts)
    assert got.dtype == np.uint32
    assert np.array_equal(got, distance.taxon_counts_host(tmparr, starts))
    assert np.array_equal(got, tm.counts(tmparr, starts))
    return got


# -- tile edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 5, 63, 64, 65, 129])
def test_tile_edges(engine, T):
    tmparr, locus = random_matrix(T, 2100, T)
    engine.set_data(tmparr, locus)
    assert_three_agree(engine, tmparr)
    assert_three_agree(engine, tmparr, [0, 700, 1411, 2100])
    nt = (T + 63) // 64
    assert engine.taxon_counts_stats()["tile_pairs"] == nt * (nt + 1) // 2


# -- word and chunk edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 31, 32, 33, 63, 64, 65, 511, 512, 513])
def test_word_edges(engine, S):
    tmparr, locus = random_matrix(5, S, 1000 + S)
    engine.set_data(tmparr, locus)
    assert_three_agree(engine, tmparr)
    st = engine.taxon_counts_stats()
    assert st["work_items"] == ((S - 1) // 64) // st["slice_words"] + 1 and st["tile_pairs"] == 1


def test_slice_edges(engine):
    tmparr, locus = random_matrix(5, 1, 0)
    engine.set_data(tmparr, locus)
    engine.taxon_counts()
    slice_sites = 64 * engine.taxon_counts_stats()["slice_words"]
    assert slice_sites % 512 == 0                                  # a multiple of the staged chunk of 8 words
    for S, items in ((slice_sites - 1, 1), (slice_sites, 1), (slice_sites + 1, 2), (3 * slice_sites + 65, 4)):
        tmparr, locus = random_matrix(5, S, S)
        engine.set_data(tmparr, locus)
        assert_three_agree(engine, tmparr)
        st = engine.taxon_counts_stats()
        assert st["work_items"] == items and st["chunks"] == 1 and st["chunk_blocks"] == 1
        # a block that starts inside a word: the slices are counted from its first word
        assert_three_agree(engine, tmparr, [63, S])
        assert engine.taxon_counts_stats()["work_items"] == ((S - 1) // 64 - 0) // (slice_sites // 64) + 1


def test_slice_length_has_no_say(engine):
    tmparr, locus = random_matrix(66, 5000, 66)
    engine.set_data(tmparr, locus)
    starts = [3, 1000, 1001, 4097, 5000]
    want = assert_three_agree(engine, tmparr, starts)
    default = engine.taxon_counts_stats()["slice_words"]
    try:
        for words in (8, 16, 128):
            engine.set_option("taxdist_slice_words", words)
            assert np.array_equal(engine.taxon_counts(starts), want)
            assert engine.taxon_counts_stats()["slice_words"] == words
        for bad in (4, 12, -8):
            with pytest.raises(Exception, match="taxdist_slice_words"):
                engine.set_option("taxdist_slice_words", bad)
    finally:
        engine.set_option("taxdist_slice_words", 0)
    assert engine.taxon_counts(starts) is not None and engine.taxon_counts_stats()["slice_words"] == default


# -- blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_with_tiling(engine, name):
    g = load_golden(name)
    engine.set_data(g["tmparr"], g["tmpmap"])
    S = g["tmparr"].shape[1]
    tiled = assert_three_agree(engine, g["tmparr"], tm.tiling(S))
    whole = assert_three_agree(engine, g["tmparr"])
    assert np.array_equal(tiled.astype(np.int64).sum(axis=0), whole[0])


@pytest.mark.parametrize("starts", [
    [70, 75], [64, 65, 127, 128], [0, 1],                          # both cuts inside one 64-site word
    [0, 32, 64, 96, 128, 192, 256],                                # cuts on 32- and 64-site boundaries
    [2, 70, 200, 257], [3, 60, 66, 67, 130, 190],                  # blocks with gaps
], ids=str)
def test_block_shapes(engine, starts):
    g = load_golden("sparse_T10_S257")
    engine.set_data(g["tmparr"], g["tmpmap"])
    assert_three_agree(engine, g["tmparr"], starts)


def test_most_blocks(engine):
    tmparr, locus = random_matrix(4, 5000, 4096)
    engine.set_data(tmparr, locus)
    starts = np.concatenate([np.arange(4096), [5000]]).astype(np.int64)
    assert_three_agree(engine, tmparr, starts)
    assert engine.taxon_counts_stats()["work_items"] == 4095 + (5000 // 64 - 4095 // 64) // engine.taxon_counts_stats()["slice_words"] + 1


def test_chunks_of_blocks(engine):
    tmparr, locus = random_matrix(70, 3000, 70)
    engine.set_data(tmparr, locus)
    starts = np.linspace(0, 3000, 12).astype(np.int64)              # 11 blocks of 70 x 70 x 16 = 78 400 bytes
    want = assert_three_agree(engine, tmparr, starts)
    one = engine.taxon_counts_stats()
    assert one["chunks"] == 1 and one["chunk_blocks"] == 11
    try:
        for limit, per in ((3 * 78400 + 5, 3), (78400, 1), (100, 1)):
            engine.set_option("taxdist_scratch_bytes", limit)
            assert np.array_equal(engine.taxon_counts(starts), want)
            st = engine.taxon_counts_stats()
            assert st["chunk_blocks"] == per and st["chunks"] == -(-11 // per) and st["work_items"] == one["work_items"]
        with pytest.raises(Exception, match="taxdist_scratch_bytes"):
            engine.set_option("taxdist_scratch_bytes", -1)
    finally:
        engine.set_option("taxdist_scratch_bytes", 0)
    assert np.array_equal(engine.taxon_counts(starts), want) and engine.taxon_counts_stats()["chunks"] == 1


# -- cross-check with the block rows of section 20 -------------------------------------------------------------------------
def test_cross_check_with_pattern_blocks(engine):
    from tetrad_amd.patterns import CLASS_STRINGS
    tmparr, locus = random_matrix(4, 3000, 20)
    tmparr[2:] = np.random.default_rng(21).integers(0, 4, size=(2, 3000), dtype=np.uint8)      # taxa 2 and 3 never missing
    engine.set_data(tmparr, locus)
    starts = [0, 100, 1000, 1001, 3000]
    engine.set_option("count_invariant", 1)
    try:
        rows = engine.patterns_blocks(np.array([[0, 1, 2, 3]], np.uint32), starts)[0].astype(np.int64)     # [B, 16]
        counts = engine.taxon_counts(starts).astype(np.int64)
    finally:
        engine.set_option("count_invariant", 0)
    assert np.array_equal(counts[:, 0, 1, 0], rows[:, :15].sum(axis=1))
    differ = [k for k, s in enumerate(CLASS_STRINGS) if s[0] != s[1]]
    assert [CLASS_STRINGS[k] for k in differ] == ["0100", "0101", "0102", "0110", "0111", "0112", "0120", "0121", "0122", "0123"]
    assert np.array_equal(counts[:, 0, 1, 1], rows[:, differ].sum(axis=1))
    assert np.array_equal(engine.taxon_counts(starts), counts)                               # count_invariant has no say


# -- device-built replicates ---------------------------------------------------------------------------------------------
def test_counts_of_a_bootstrap_replicate():
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    rng = np.random.default_rng(3)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        for pack in (0, 1):                                         # the natural layout is read either way
            eng.set_option("boot_pack", pack)
            S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))
            tmparr, tmpmap = eng.get_data()
            assert tmparr.shape[1] == S
            for starts in (None, tm.tiling(S), patterns.locus_blocks(tmpmap, 9)):
                assert_three_agree(eng, tmparr, starts)
            with pytest.raises(Exception, match="past the S="):
                eng.taxon_counts([0, S + 1])


# -- streams -------------------------------------------------------------------------------------------------------------
def test_two_streams_two_buffers(engine):
    import torch
    g = load_golden("dense_T8_S400")
    engine.set_data(g["tmparr"], g["tmpmap"])
    first, second = tm.tiling(400), np.array([10, 50, 390], np.int64)
    want_a, want_b = engine.taxon_counts(first), engine.taxon_counts(second)
    d_a = torch.full((len(first) - 1, 8, 8, 4), -1, dtype=torch.int32, device="cuda")
    d_b = torch.full((2, 8, 8, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # the second call overwrites the work items of the first: the stream rule keeps the first call's kernels in front
    engine.taxon_counts_dev(first, d_a.data_ptr(), s1.cuda_stream)
    engine.taxon_counts_dev(second, d_b.data_ptr(), s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), want_a) and np.array_equal(want_a, tm.counts(g["tmparr"], first))
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), want_b) and np.array_equal(want_b, tm.counts(g["tmparr"], second))
    d_one = torch.full((1, 8, 8, 4), -1, dtype=torch.int32, device="cuda")
    engine.taxon_counts_dev(None, d_one.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_one.cpu().numpy().view(np.uint32), tm.counts(g["tmparr"]))


def test_ordered_behind_a_bootstrap_on_another_stream():
    import torch
    from tetrad_amd import bootstrap
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    rng = np.random.default_rng(8)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))                       # a first replicate, resident
        build, count = torch.cuda.Stream(), torch.cuda.Stream()
        S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng), stream=build.cuda_stream)
        d_out = torch.full((1, 7, 7, 4), -1, dtype=torch.int32, device="cuda")
        eng.taxon_counts_dev(None, d_out.data_ptr(), count.cuda_stream)
        count.synchronize()
        tmparr, _ = eng.get_data()
        assert tmparr.shape[1] == S
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), tm.counts(tmparr))


# -- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    import torch
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("edge_T7_S130")
    S = 130
    engine.set_data(g["tmparr"], g["tmpmap"])
    lib, h = engine._lib, engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = np.array([0, 50, 130], np.int64)

    def host(starts_, B=None):
        st = np.ascontiguousarray(starts_, np.int64)
        nb = len(st) - 1 if B is None else B
        out = np.full((max(nb, 1), 7, 7, 4), 0xABABABAB, np.uint32)
        rc = lib.tq_taxon_counts(h, p(st), nb, p(out))
        return rc, bool((out == 0xABABABAB).all()), lib.tq_last_error(h)

    assert host(good)[:2] == (0, False)
    long_starts = np.arange(4098, dtype=np.int64)
    for args, word in [((good, 0), b"B=0"), ((long_starts,), b"B=4097"), (([0, 50, 50, 130],), b"not above"),
                       (([0, 60, 50, 130],), b"not above"), (([-1, 50, 130],), b"negative"), (([0, 50, S + 1],), b"past the S=")]:
        rc, untouched, msg = host(*args)
        assert rc == -1 and untouched and word in msg and msg.startswith(b"tq_taxon_counts:"), (word, msg)
    out = np.zeros((2, 7, 7, 4), np.uint32)
    assert lib.tq_taxon_counts(h, None, 2, p(out)) == -1 and lib.tq_taxon_counts(h, p(good), 2, None) == -1
    assert lib.tq_taxon_counts(None, p(good), 2, p(out)) == -1 and lib.tq_taxon_counts_stats(None, p(out)) == -1
    with QuartetEngine(0) as fresh:                                 # no data
        with pytest.raises(TetradHipError, match="TQ_ERR_NO_DATA"):
            fresh.taxon_counts(good)
        with pytest.raises(TetradHipError, match="TQ_ERR_NO_DATA"):
            fresh.taxon_counts_dev(good, 256)
    d_out = torch.full((2, 7, 7, 4), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    for kwargs in (dict(block_starts=[0, 50, 50, 130]), dict(block_starts=[0, 50, S + 1]), dict(block_starts=[-1, 5]),
                   dict(block_starts=long_starts), dict(d_out=d_out.data_ptr() + 4), dict(d_out=d_out.data_ptr() + 8), dict(d_out=0)):
        a = dict(block_starts=good, d_out=d_out.data_ptr(), stream=cs)
        a.update(kwargs)
        with pytest.raises(TetradHipError, match="TQ_ERR_INVALID_ARG"):
            engine.taxon_counts_dev(**a)
    with pytest.raises(TetradHipError, match="16-byte aligned"):
        engine.taxon_counts_dev(good, d_out.data_ptr() + 8, cs)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()


def test_no_timing_mark(engine):
    g = load_golden("edge_T7_S130")
    engine.set_data(g["tmparr"], g["tmpmap"])
    engine.timing_enable(True)
    try:
        engine.timing_read_split()
        engine.taxon_counts([0, 50, 130])
        total, scan, svd, calls = engine.timing_read_split()
        assert calls == 0 and total == 0.0
    finally:
        engine.timing_enable(False)


# -- end to end ------------------------------------------------------------------------------------------------------------
def test_bootstrap_nj_trees_into_a_consensus(engine):
    from tetrad_amd import bootstrap, distance
    from tetrad_amd.consensus import Consensus
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    with QuartetEngine(0) as eng, Consensus(7, engine=eng) as cons, Consensus(7) as by_hand:
        parents = distance.bootstrap_nj_trees(eng, g["seqarr"], g["spans"], 6, np.random.default_rng(5), model="p", consensus=cons)
        assert len(parents) == 6 and cons.ntrees == 6
        # the same replicates drawn by hand, counted by the model
        rng = np.random.default_rng(5)
        eng.set_source(g["seqarr"], g["spans"])
        for k in range(6):
            bootstrap.resample_tmp_database(eng, rng)
            c = tm.counts(eng.get_data()[0])[0].astype(np.int64)
            want = tm.nj((c[..., 1] / c[..., 0]).tolist())[0]
            assert parents[k].tolist() == want
            by_hand.add_parents([np.array(want, np.int32)])
        a, b = cons.splits(), by_hand.splits()
        key = lambda s: sorted((m.tobytes(), int(c)) for m, c in zip(s[0], s[1]))
        assert key(a) == key(b) and a[2] == b[2] == 6


def test_polish_from_the_nj_tree(engine):
    from tetrad_amd import distance, synth
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.qmc import Supertree
    T = 12
    tmparr, tmpmap = synth.simulate_tmparr(T, 3000, seed=11)
    engine.set_data(tmparr, tmpmap)
    quartets = synth.all_quartets(T)
    rstat, rscor, flags = engine.resolve(quartets, False)
    d = distance.distances(engine.taxon_counts()[0], "jc")
    assert np.isfinite(d).all()
    start = distance.nj_parents(d)
    with Supertree(T, len(quartets), 1, engine=engine) as st:
        st.add(quartets, rscor, rstat, flags)
        nwk, trace = st.polish(start)
        assert newick_to_parent(nwk)[1] == T and trace.converged
        assert int(st.fit(nwk)["k_satisfied"]) >= int(st.fit(start)["k_satisfied"])


def test_run_distance_tree(engine):
    from tetrad_amd import distance, patterns, synth
    from tetrad_amd.concordance import newick_to_parent
    T, S = 12, 4000
    tmparr, tmpmap = synth.simulate_tmparr(T, S, 0, p=0.05, missing=0.10)
    children, root = synth.random_tree_children(T, np.random.default_rng(0))
    true = tm.splits(tm.children_to_parent(children, root, T), T)
    newick, counts = distance.run_distance_tree(engine, tmparr, tmpmap, model="jc", nblocks=50)
    assert np.array_equal(counts, tm.counts(tmparr, patterns.locus_blocks(tmpmap, 50)))
    assert tm.splits(newick_to_parent(newick)[0], T) == true
    import re
    assert [int(x) for x in re.findall(r"\)(\d+):", newick)] == [100] * (T - 3)
