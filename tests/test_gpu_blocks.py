"""GPU: class rows per block of sites against an independent model, against the histogram scan on the block's column
slice and on the whole matrix; the device jackknife against the host execution and Python floats; and
`run_dstat_jackknife` end to end."""
import ctypes
import math
from itertools import combinations

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import patterns_model as pm

pytestmark = pytest.mark.gpu

GOLDENS = ["tiny_T5_S37", "one_site_T5_S1", "edge_T7_S130", "sparse_T10_S257", "dense_T8_S400", "carry_T6_S2500"]


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def all_sets(T):
    return np.array(list(combinations(range(T), 4)), np.uint32)


def tiling(S):
    """A tiling of [0, S) with cuts off and on the 32-site words (as far as S allows)."""
    cuts = sorted({c for c in (1, 5, 31, 32, 33, 64, 100, 129, 256, 300, 2047, 2048, 2049) if c < S})
    return np.array([0] + cuts + [S], np.int64)


_MODEL = {}


def model_rows(name, starts, inv):
    """bm.block_rows of every set of a golden, computed once per (golden, blocks, count_invariant)."""
    key = (name, tuple(int(v) for v in starts), bool(inv))
    if key not in _MODEL:
        g = load_golden(name)
        _MODEL[key] = bm.block_rows(g["tmparr"], all_sets(g["tmparr"].shape[0]), starts, inv)
    return _MODEL[key]


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_against_three_yardsticks(engine, name, inv):
    g = load_golden(name)
    tmparr, tmpmap = g["tmparr"], g["tmpmap"]
    T, S = tmparr.shape
    sets = all_sets(T)
    starts = tiling(S)
    B = len(starts) - 1
    engine.set_option("count_invariant", inv)
    try:
        engine.set_data(tmparr, tmpmap)
        rows = engine.patterns_blocks(sets, starts)
        whole = engine.patterns(sets, False)
        one = engine.patterns_blocks(sets, [0, S])
        assert rows.dtype == np.uint32 and rows.shape == (len(sets), B, 16)
        # 1. the model on the raw columns
        assert np.array_equal(rows, model_rows(name, starts, inv))
        assert np.array_equal(one, model_rows(name, [0, S], inv))
        assert bool(rows[:, :, 0].any()) == bool(inv and model_rows(name, starts, 1)[:, :, 0].any())
        # 3. a tiling sums to the row of the histogram scan, and B = 1 is that row
        assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), whole.astype(np.uint64))
        assert np.array_equal(one[:, 0], whole)
        # 2. the histogram scan on the block's column slice
        for j in range(B):
            s0, s1 = int(starts[j]), int(starts[j + 1])
            engine.set_data(np.ascontiguousarray(tmparr[:, s0:s1]), np.ascontiguousarray(tmpmap[s0:s1]))
            assert np.array_equal(engine.patterns(sets, False), rows[:, j]), (j, s0, s1)
    finally:
        engine.set_option("count_invariant", 0)


def shape_cases(S, tmpmap):
    from tetrad_amd import patterns
    cases = {
        "whole": [0, S],
        "one_site_blocks": list(range(90, 131)),                     # 40 blocks of one site across a word edge
        "inside_one_word": [45, 49],                                 # sites 45, 47 and 48 are counted
        "both_cuts_in_one_word": [33, 63],
        "last_word": [S - 3, S],                                     # inside the last, partial word
        "word_edges": [0, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 2047, 2048, 2049, S],
        "longer_than_16_words": [5, 1200, S],                        # 38 and 41 words: a lane takes up to three
        "head_and_tail_uncovered": [17, 400, 900, 2400],
        "B7": np.linspace(0, S, 8).astype(np.int64),
        "B64": np.linspace(3, S - 2, 65).astype(np.int64),
        "B65": np.linspace(0, S, 66).astype(np.int64),
        "locus_blocks": patterns.locus_blocks(tmpmap, 10),
    }
    return cases


SHAPES = ["whole", "one_site_blocks", "inside_one_word", "both_cuts_in_one_word", "last_word", "word_edges",
          "longer_than_16_words", "head_and_tail_uncovered", "B7", "B64", "B65", "locus_blocks"]


@pytest.mark.parametrize("shape", SHAPES)
def test_block_shapes(engine, shape):
    """Where the range masks and the lane loop can go wrong, on 2 500 sites (78 words and four sites)."""
    g = load_golden("carry_T6_S2500")
    tmparr, tmpmap = g["tmparr"], g["tmpmap"]
    starts = np.asarray(shape_cases(tmparr.shape[1], tmpmap)[shape], np.int64)
    assert (np.diff(starts) > 0).all()
    engine.set_data(tmparr, tmpmap)
    rows = engine.patterns_blocks(all_sets(6), starts)
    assert np.array_equal(rows, model_rows("carry_T6_S2500", starts, 0))
    assert rows[:, :, 15].any()                                      # the case looks at counted sites


@pytest.mark.parametrize("Q", [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_with_a_canary(engine, Q):
    """Sixteen lanes per item, four items per wavefront, sixteen per workgroup; B = 3 makes Q B odd for odd Q."""
    import torch
    g = load_golden("sparse_T10_S257")
    starts = np.array([2, 70, 200, 257], np.int64)
    want = model_rows("sparse_T10_S257", starts, 0)[:Q]
    sets = all_sets(10)[:Q]
    engine.set_data(g["tmparr"], g["tmpmap"])
    assert np.array_equal(engine.patterns_blocks(sets, starts), want)
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    d_out = torch.full((Q * 3 + 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_blocks_dev(d_sets.data_ptr(), Q, starts, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:Q * 3].reshape(Q, 3, 16), want) and (out[Q * 3:] == 0xFFFFFFFF).all()


def test_host_form_chunks_by_batch(engine):
    g = load_golden("sparse_T10_S257")
    starts = np.array([2, 70, 200, 257], np.int64)
    engine.set_data(g["tmparr"], g["tmpmap"])
    want = model_rows("sparse_T10_S257", starts, 0)
    for batch in (100, 2):                                           # chunks of 33 sets; B above batch: one set a chunk
        engine.set_option("batch", batch)
        try:
            assert np.array_equal(engine.patterns_blocks(all_sets(10), starts), want)
        finally:
            engine.set_option("batch", 0)


def test_packed_layout_is_not_read(engine):
    g = load_golden("sparse_T10_S257")
    starts = tiling(257)
    engine.set_option("site_pack", 1)
    try:
        engine.set_data(g["tmparr"], g["tmpmap"])
        assert engine.site_pack_state()[0]                           # the packed set exists
        rows = engine.patterns_blocks(all_sets(10), starts)
    finally:
        engine.set_option("site_pack", -1)
    assert np.array_equal(rows, model_rows("sparse_T10_S257", starts, 0))


def test_rows_of_a_bootstrap_replicate():
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    sets = all_sets(7)
    rng = np.random.default_rng(3)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        for pack in (0, 1):
            eng.set_option("boot_pack", pack)
            S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))
            tmparr, tmpmap = eng.get_data()
            assert tmparr.shape[1] == S
            for starts in (tiling(S), patterns.locus_blocks(tmpmap, 9)):
                assert np.array_equal(eng.patterns_blocks(sets, starts), bm.block_rows(tmparr, sets, starts))
            with pytest.raises(Exception, match="past the S="):
                eng.patterns_blocks(sets, [0, S + 1])


def test_two_calls_on_another_stream(engine):
    import torch
    g = load_golden("dense_T8_S400")
    sets = all_sets(8)
    engine.set_data(g["tmparr"], g["tmpmap"])
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    first, second = tiling(400), np.array([10, 50, 390], np.int64)
    d_whole = torch.empty((len(sets), 16), dtype=torch.int32, device="cuda")
    d_a = torch.zeros((len(sets), len(first) - 1, 16), dtype=torch.int32, device="cuda")
    d_b = torch.zeros((len(sets), 2, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    engine.patterns_dev(d_sets.data_ptr(), len(sets), False, d_whole.data_ptr(), torch.cuda.current_stream().cuda_stream)
    side = torch.cuda.Stream()
    # the second call overwrites the boundaries of the first: stream order keeps the first call's kernel in front
    engine.patterns_blocks_dev(d_sets.data_ptr(), len(sets), first, d_a.data_ptr(), side.cuda_stream)
    engine.patterns_blocks_dev(d_sets.data_ptr(), len(sets), second, d_b.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), model_rows("dense_T8_S400", first, 0))
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), model_rows("dense_T8_S400", second, 0))
    assert np.array_equal(d_whole.cpu().numpy().view(np.uint32), pm.model_classes(g["tmparr"], g["tmpmap"], sets, False))


def test_refusals(engine):
    import torch
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("edge_T7_S130")
    sets = all_sets(7)
    S = 130
    engine.set_data(g["tmparr"], g["tmpmap"])
    lib, h = engine._lib, engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = np.array([0, 50, 130], np.int64)

    def host(sets_, starts_, B=None):
        out = np.full((len(sets_), (len(starts_) - 1) if B is None else max(B, 1), 16), 0xABABABAB, np.uint32)
        st = np.ascontiguousarray(starts_, np.int64)
        rc = lib.tq_patterns_blocks(h, p(np.ascontiguousarray(sets_, np.uint32)), len(sets_), p(st),
                                    len(st) - 1 if B is None else B, p(out))
        return rc, bool((out == 0xABABABAB).all()), lib.tq_last_error(h)

    assert host(sets, good)[0] == 0
    bad_t = sets.copy()
    bad_t[3, 3] = 7
    bad_order = sets.copy()
    bad_order[5] = bad_order[5][[0, 2, 1, 3]]
    long_starts = np.arange(4098, dtype=np.int64)                    # B = 4097 (and past S)
    for args, word in [((bad_t, good), b"index >= T"), ((bad_order, good), b"not strictly ascending"),
                       ((sets, good, 0), b"B=0"), ((sets, long_starts), b"B=4097"),
                       ((sets, [0, 50, 50, 130]), b"not above"), ((sets, [0, 60, 50, 130]), b"not above"),
                       ((sets, [-1, 50, 130]), b"negative"), ((sets, [0, 50, S + 1]), b"past the S=")]:
        rc, untouched, msg = host(*args)
        assert rc == -1 and untouched and word in msg, (word, msg)
    # the row check is one function for every width and kind of set: its two texts in full
    assert host(bad_t, good)[2] == b"tq_patterns_blocks: row 3 has an index >= T=7"
    assert host(bad_order, good)[2] == b"tq_patterns_blocks: row 5 (0, 3, 1, 5) is not strictly ascending"
    assert lib.tq_patterns_blocks(h, None, 0, p(good), 2, None) == 0                     # Q = 0 is valid
    assert lib.tq_patterns_blocks(h, None, 0, None, 2, None) == -1
    assert lib.tq_patterns_blocks(h, None, -1, p(good), 2, None) == -1
    assert lib.tq_patterns_blocks(None, None, 0, p(good), 2, None) == -1
    with QuartetEngine(0) as fresh:                                                     # no data
        with pytest.raises(TetradHipError, match="TQ_ERR_NO_DATA"):
            fresh.patterns_blocks(sets, good)
    # the device form: a taxon >= T gives zero rows, everything else is refused before anything is launched
    d_sets = torch.from_numpy(bad_t.view(np.int32)).cuda()
    d_out = torch.full((len(sets), 2, 16), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    engine.patterns_blocks_dev(d_sets.data_ptr(), len(sets), good, d_out.data_ptr(), cs)
    out = d_out.cpu().numpy().view(np.uint32)
    want = bm.block_rows(g["tmparr"], sets, good)
    want[3] = 0
    assert np.array_equal(out, want)
    d_out.fill_(-1)
    for kwargs in (dict(block_starts=[0, 50, 50, 130]), dict(block_starts=[0, 50, S + 1]), dict(block_starts=[-1, 5]),
                   dict(block_starts=long_starts), dict(d_sets=d_sets.data_ptr() + 4), dict(d_classes=d_out.data_ptr() + 8)):
        a = dict(d_sets=d_sets.data_ptr(), Q=len(sets), block_starts=good, d_classes=d_out.data_ptr(), stream=cs)
        a.update(kwargs)
        with pytest.raises(TetradHipError, match="TQ_ERR_INVALID_ARG"):
            engine.patterns_blocks_dev(**a)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()


def test_locus_column_has_no_say(engine):
    """Subsample mode would refuse this locus column (an id in two runs); block rows are full mode only and do not read
    it, and the scan options leave them alone."""
    g = load_golden("edge_T7_S130")
    sets = all_sets(7)
    locus = (np.arange(130) % 3).astype(np.uint32)
    engine.set_data(g["tmparr"], locus)
    with pytest.raises(Exception, match="TQ_ERR_LOCUS_ORDER"):
        engine.patterns(sets, True)
    starts = tiling(130)
    want = model_rows("edge_T7_S130", starts, 0)
    assert np.array_equal(engine.patterns_blocks(sets, starts), want)
    engine.set_option("scan_method", 2)                              # a timing-diagnostic mode of the scans
    try:
        assert np.array_equal(engine.patterns_blocks(sets, starts), want)
    finally:
        engine.set_option("scan_method", -1)


@pytest.mark.parametrize("B", [1, 2, 3, 50, 4096])
def test_device_jackknife(engine, B):
    import torch
    from tetrad_amd import patterns
    N = 65 if B == 4096 else 1000
    rows, set_of, ia, ib = bm.jackknife_case(N, B)
    want = bm.jackknife_model(rows, set_of, ia, ib)
    assert np.array_equal(bm.bits(patterns.dstat_jackknife(rows, set_of, ia, ib)), bm.bits(want))
    # three tests out of range: their rows stay as they were
    skip = [t for t in (10, 20, 30) if t < N]
    set_of, ia, ib = set_of.copy(), ia.copy(), ib.copy()
    set_of[10], ia[20], ib[30] = rows.shape[0], 15, 255
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    d_set_of = torch.from_numpy(set_of.view(np.int32)).cuda()
    d_ia, d_ib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    d_out = torch.full((N + 1, 4), 2.5, dtype=torch.float64, device="cuda")
    engine.dstat_jackknife_dev(d_rows.data_ptr(), rows.shape[0], B, d_set_of.data_ptr(), d_ia.data_ptr(), d_ib.data_ptr(), N,
                               d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = d_out.cpu().numpy()
    keep = np.ones(N, bool)
    keep[skip] = False
    assert (got[:N][~keep] == 2.5).all() and (got[N] == 2.5).all()
    assert np.array_equal(bm.bits(got[:N][keep]), bm.bits(want[keep]))
    with pytest.raises(Exception, match="B="):
        engine.dstat_jackknife_dev(d_rows.data_ptr(), rows.shape[0], 4097, d_set_of.data_ptr(), d_ia.data_ptr(),
                                   d_ib.data_ptr(), N, d_out.data_ptr(), 0)


_TREE = {}


def tree_reference():
    """tree_T12_S2000, every test with outgroup 0, ten locus blocks: the model chain, once."""
    if not _TREE:
        from tetrad_amd import patterns
        g = load_golden("tree_T12_S2000")
        tmparr, tmpmap = g["tmparr"], g["tmpmap"]
        tests = patterns.tests_with_outgroup(12, 0)
        starts = patterns.locus_blocks(tmpmap, 10)
        sets, set_of, idx = patterns._role_classes(tests, (patterns.ABBA, patterns.BABA, patterns.BBAA))
        rows = bm.block_rows(tmparr, sets, starts)
        jk = bm.jackknife_model(rows, set_of, idx[:, 0], idx[:, 1])
        _TREE.update(tmparr=tmparr, tmpmap=tmpmap, tests=tests, starts=starts, sets=sets, set_of=set_of, idx=idx, rows=rows,
                     jk=jk)
    return _TREE


@pytest.mark.parametrize("chunk", [1 << 16, 100])
def test_run_dstat_jackknife_end_to_end(chunk):
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    r = tree_reference()
    tmparr, tmpmap, tests = r["tmparr"], r["tmpmap"], r["tests"]
    assert len(r["sets"]) == 165 and len(tests) == 495 and len(r["starts"]) == 11       # chunk 100: 100 + 65 sets
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)].copy()
    seqarr[tmparr > 3] = ord("N")
    with QuartetEngine(0) as eng:
        res = patterns.run_dstat_jackknife(eng, tmparr, tmpmap, tests, nblocks=10, chunk=chunk)
        again = patterns.run_dstat_jackknife(eng, None, None, tests, block_starts=r["starts"], chunk=chunk, resident=True)
        boot = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, bootstrap.get_spans(tmpmap), tests, 0)
    assert res.dtype == patterns.JACKKNIFE_DTYPE and len(res) == 495
    assert res.tobytes() == again.tobytes()
    sums = r["rows"].sum(axis=1, dtype=np.int64)
    set_of, idx, jk = r["set_of"].astype(np.int64), r["idx"].astype(np.int64), r["jk"]
    t = np.arange(495)
    assert np.array_equal(res["abba"], sums[set_of, idx[:, 0]]) and np.array_equal(res["baba"], sums[set_of, idx[:, 1]])
    assert np.array_equal(res["bbaa"], sums[set_of, idx[:, 2]]) and np.array_equal(res["nsites"], sums[set_of, 15])
    for k in range(495):
        assert (res["abba"][k], res["baba"][k]) == pm.direct_abba_baba(tmparr, tests[k])
    assert np.array_equal(bm.bits(res["D"]), bm.bits(jk[:, 1]))
    assert np.array_equal(bm.bits(res["D"]), bm.bits(boot["D"]))
    for f in ("abba", "baba", "bbaa", "nsites"):
        assert np.array_equal(res[f], boot[f])
    assert np.array_equal(res["jk_blocks"], jk[:, 0].astype(np.int64))
    assert np.array_equal(bm.bits(res["jk_mean"]), bm.bits(jk[:, 2]))
    se = [math.sqrt(v) if not math.isnan(v) else math.nan for v in jk[:, 3]]
    assert np.array_equal(bm.bits(res["jk_se"]), bm.bits(se))
    Z = [float(d) / s if s > 0 else math.nan for d, s in zip(jk[:, 1], se)]
    assert np.array_equal(bm.bits(res["Z"]), bm.bits(Z))
    assert np.isfinite(res["Z"]).sum() > 400                                              # the case is not degenerate
