"""GPU: five-taxon class rows per block of sites against an independent model, on a designed matrix of all 1024 patterns
and against the four-taxon kernel; the device jackknife on sums of slots against the host execution and Python floats;
and `run_quintet_jackknife` end to end.  Everything is bit-exact."""
import ctypes
import math
from itertools import combinations, product

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import quintets_model as qm
from test_gpu_blocks import SHAPES, shape_cases, tiling

pytestmark = pytest.mark.gpu

GOLDENS = ["tiny_T5_S37", "one_site_T5_S1", "edge_T7_S130", "sparse_T10_S257", "dense_T8_S400", "carry_T6_S2500"]
MISSING = 78


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def all_sets5(T):
    return np.array(list(combinations(range(T), 5)), np.uint32)


def plain_map(S, width=8):
    return np.stack([np.arange(S) // width, np.arange(S)], axis=1).astype(np.uint32)


_MODEL = {}


def model_rows(name, starts):
    """qm.block_rows of every five-set of a golden, computed once per (golden, blocks)."""
    key = (name, tuple(int(v) for v in starts))
    if key not in _MODEL:
        g = load_golden(name)
        _MODEL[key] = qm.block_rows(g["tmparr"], all_sets5(g["tmparr"].shape[0]), starts)
    return _MODEL[key]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_against_the_model(engine, name):
    g = load_golden(name)
    T, S = g["tmparr"].shape
    sets, starts = all_sets5(T), tiling(S)
    engine.set_data(g["tmparr"], g["tmpmap"])
    rows = engine.patterns_quintet_blocks(sets, starts)
    one = engine.patterns_quintet_blocks(sets, [0, S])
    assert rows.dtype == np.uint32 and rows.shape == (len(sets), len(starts) - 1, 16)
    assert np.array_equal(rows, model_rows(name, starts))
    assert np.array_equal(one, model_rows(name, [0, S]))
    assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), one[:, 0].astype(np.uint64))      # a tiling sums to B = 1
    assert np.array_equal(rows[:, :, 0], rows[:, :, 1:].sum(axis=2, dtype=np.uint32))
    engine.set_option("count_invariant", 1)                                                    # is not read
    try:
        assert np.array_equal(engine.patterns_quintet_blocks(sets, starts), rows)
    finally:
        engine.set_option("count_invariant", 0)


def designed_matrix():
    """T = 5, S = 6144: all 1024 patterns as columns, then the 1024 again with taxon t missing, for t = 0..4."""
    pats = np.array(list(product(range(4), repeat=5)), np.uint8).T                             # [5, 1024]
    parts = [pats]
    for t in range(5):
        p = pats.copy()
        p[t] = MISSING
        parts.append(p)
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def test_designed_matrix_of_all_patterns(engine):
    tmparr = designed_matrix()
    assert tmparr.shape == (5, 6144)
    sets = all_sets5(5)
    engine.set_data(tmparr, plain_map(6144))
    whole = engine.patterns_quintet_blocks(sets, [0, 6144])
    assert whole[0, 0].tolist() == [180] + [12] * 15
    assert np.array_equal(engine.patterns_quintet_blocks(sets, [0, 1024]), whole)              # a missing taxon: nowhere
    assert not engine.patterns_quintet_blocks(sets, [1024, 6144]).any()
    # one-site blocks (at most 4096 a call): every block row is the model's, and every class is met
    seen = np.zeros(16, np.int64)
    for lo, hi in ((0, 3072), (3072, 6144)):
        starts = np.arange(lo, hi + 1, dtype=np.int64)
        rows = engine.patterns_quintet_blocks(sets, starts)
        assert np.array_equal(rows, qm.block_rows(tmparr, sets, starts))
        seen += rows[0].sum(axis=0, dtype=np.int64)
    assert seen.tolist() == [180] + [12] * 15
    # the library's table says the same of the first 1024 columns
    from tetrad_amd import quintets
    first = engine.patterns_quintet_blocks(sets, np.arange(0, 1025, dtype=np.int64))[0]
    table = quintets.class_table()
    assert np.array_equal(first[:, 0], (table != 0).astype(np.uint32))
    assert all(first[p, table[p]] == 1 for p in range(1024) if table[p])


def two_base_matrix():
    rng = np.random.default_rng(20)
    tmparr = rng.integers(0, 2, size=(7, 2500)).astype(np.uint8)
    hole = rng.random((6, 2500)) < 0.10
    tmparr[:6][hole] = MISSING
    return tmparr


@pytest.mark.parametrize("shape", SHAPES)
def test_block_shapes(engine, shape):
    """Where the range masks and the lane loop can go wrong, on 2 500 sites (78 words and four sites)."""
    g = load_golden("carry_T6_S2500")
    starts = np.asarray(shape_cases(2500, g["tmpmap"])[shape], np.int64)
    assert (np.diff(starts) > 0).all()
    engine.set_data(g["tmparr"], g["tmpmap"])
    rows = engine.patterns_quintet_blocks(all_sets5(6), starts)
    assert np.array_equal(rows, model_rows("carry_T6_S2500", starts))


@pytest.mark.parametrize("shape", SHAPES)
def test_block_shapes_on_a_dense_matrix(engine, shape):
    """The golden above has few biallelic five-taxon sites (its shortest blocks hold none): the same cuts on the two-base
    matrix below, where every block of every case counts some."""
    tmparr, tmpmap = two_base_matrix(), plain_map(2500)
    starts = np.asarray(shape_cases(2500, tmpmap)[shape], np.int64)
    engine.set_data(tmparr, tmpmap)
    sets = all_sets5(7)
    rows = engine.patterns_quintet_blocks(sets, starts)
    assert np.array_equal(rows, qm.block_rows(tmparr, sets, starts))
    assert rows[:, :, 0].any(axis=0).all()                           # every block looks at counted sites


def test_2500_one_site_blocks(engine):
    g = load_golden("carry_T6_S2500")
    starts = np.arange(0, 2501, dtype=np.int64)
    engine.set_data(g["tmparr"], g["tmpmap"])
    rows = engine.patterns_quintet_blocks(all_sets5(6), starts)
    assert np.array_equal(rows, model_rows("carry_T6_S2500", starts)) and rows[:, :, 0].any()


# ---- against the four-taxon kernel ----

def test_cross_check_against_the_quartet_rows(engine):
    """Two bases only and taxon 6 always present: a site the quartet (a, b, c, d) counts is a five-taxon site of
    (a, b, c, d, 6), biallelic or invariant.  With m = the quartet's "differs from x0" bits, the quartet class of m is
    slot m (taxon 6 holds x0's base) plus slot m | 8 (it holds the other); class 0000 is slot 8 plus the invariant
    five-taxon sites."""
    from tetrad_amd import patterns
    tmparr = two_base_matrix()
    sets4 = np.array(list(combinations(range(6), 4)), np.uint32)
    sets5 = np.concatenate([sets4, np.full((len(sets4), 1), 6, np.uint32)], axis=1)
    starts = shape_cases(2500, plain_map(2500))["B7"]
    engine.set_data(tmparr, plain_map(2500))
    engine.set_option("count_invariant", 1)
    try:
        four = engine.patterns_blocks(sets4, starts)
    finally:
        engine.set_option("count_invariant", 0)
    five = engine.patterns_quintet_blocks(sets5, starts)
    assert (five[:, :, 1:].sum(axis=1) > 0).any(axis=0).all()                  # every slot is met by some set
    for m in range(1, 8):
        cls = patterns.CLASS_STRINGS.index("0" + "".join(str((m >> i) & 1) for i in range(3)))
        assert np.array_equal(four[:, :, cls], five[:, :, m] + five[:, :, m | 8]), m
    inv = np.array([[qm.invariant_sites(tmparr, s, int(starts[j]), int(starts[j + 1])) for j in range(7)] for s in sets5])
    assert inv.any()
    assert np.array_equal(four[:, :, 0], five[:, :, 8] + inv.astype(np.uint32))
    assert np.array_equal(four[:, :, 15], five[:, :, 0] + inv.astype(np.uint32))
    assert np.array_equal(five, qm.block_rows(tmparr, sets5, starts))


# ---- call behaviour ----

STARTS3 = np.array([2, 70, 200, 257], np.int64)


@pytest.mark.parametrize("Q", [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_with_a_canary(engine, Q):
    """Sixteen lanes per item, four items per wavefront, sixteen per workgroup; B = 3 makes Q B odd for odd Q."""
    import torch
    g = load_golden("sparse_T10_S257")
    want = model_rows("sparse_T10_S257", STARTS3)[:Q]
    sets = all_sets5(10)[:Q]
    engine.set_data(g["tmparr"], g["tmpmap"])
    assert np.array_equal(engine.patterns_quintet_blocks(sets, STARTS3), want)
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    d_out = torch.full((Q * 3 + 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_quintet_blocks_dev(d_sets.data_ptr(), Q, STARTS3, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:Q * 3].reshape(Q, 3, 16), want) and (out[Q * 3:] == 0xFFFFFFFF).all()


def test_host_form_chunks_by_batch(engine):
    g = load_golden("sparse_T10_S257")
    engine.set_data(g["tmparr"], g["tmpmap"])
    want = model_rows("sparse_T10_S257", STARTS3)
    for batch in (100, 2):                                           # chunks of 33 sets; B above batch: one set a chunk
        engine.set_option("batch", batch)
        try:
            assert np.array_equal(engine.patterns_quintet_blocks(all_sets5(10), STARTS3), want)
        finally:
            engine.set_option("batch", 0)


def test_packed_layout_is_not_read_and_no_call_is_timed(engine):
    g = load_golden("sparse_T10_S257")
    starts = tiling(257)
    engine.set_option("site_pack", 1)
    try:
        engine.set_data(g["tmparr"], g["tmpmap"])
        assert engine.site_pack_state()[0]                           # the packed set exists
        rows = engine.patterns_quintet_blocks(all_sets5(10), starts)
    finally:
        engine.set_option("site_pack", -1)
    assert np.array_equal(rows, model_rows("sparse_T10_S257", starts))
    engine.set_data(g["tmparr"], g["tmpmap"])
    engine.timing_enable(True)
    try:
        engine.timing_read()
        assert np.array_equal(engine.patterns_quintet_blocks(all_sets5(10), starts), rows)
        assert engine.timing_read()[1] == 0                          # no call was recorded
    finally:
        engine.timing_enable(False)


def test_rows_of_a_bootstrap_replicate():
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    sets = all_sets5(7)
    rng = np.random.default_rng(3)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        for pack in (0, 1):
            eng.set_option("boot_pack", pack)
            S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))
            tmparr, tmpmap = eng.get_data()
            assert tmparr.shape[1] == S
            for starts in (tiling(S), patterns.locus_blocks(tmpmap, 9)):
                rows = eng.patterns_quintet_blocks(sets, starts)
                assert np.array_equal(rows, qm.block_rows(tmparr, sets, starts)) and rows.any()
            with pytest.raises(Exception, match="past the S="):
                eng.patterns_quintet_blocks(sets, [0, S + 1])


def test_two_calls_on_another_stream(engine):
    import torch
    g = load_golden("dense_T8_S400")
    sets = all_sets5(8)
    engine.set_data(g["tmparr"], g["tmpmap"])
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    first, second = tiling(400), np.array([10, 50, 390], np.int64)
    d_a = torch.zeros((len(sets), len(first) - 1, 16), dtype=torch.int32, device="cuda")
    d_b = torch.zeros((len(sets), 2, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    # the second call overwrites the boundaries of the first: stream order keeps the first call's kernel in front
    engine.patterns_quintet_blocks_dev(d_sets.data_ptr(), len(sets), first, d_a.data_ptr(), side.cuda_stream)
    engine.patterns_quintet_blocks_dev(d_sets.data_ptr(), len(sets), second, d_b.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), model_rows("dense_T8_S400", first))
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), model_rows("dense_T8_S400", second))


def test_refusals(engine):
    import torch
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("edge_T7_S130")
    sets = all_sets5(7)
    S = 130
    engine.set_data(g["tmparr"], g["tmpmap"])
    lib, h = engine._lib, engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = np.array([0, 50, 130], np.int64)

    def host(sets_, starts_, B=None):
        out = np.full((len(sets_), (len(starts_) - 1) if B is None else max(B, 1), 16), 0xABABABAB, np.uint32)
        st = np.ascontiguousarray(starts_, np.int64)
        rc = lib.tq_patterns_quintet_blocks(h, p(np.ascontiguousarray(sets_, np.uint32)), len(sets_), p(st),
                                            len(st) - 1 if B is None else B, p(out))
        return rc, bool((out == 0xABABABAB).all()), lib.tq_last_error(h)

    assert host(sets, good)[0] == 0
    bad_t = sets.copy()
    bad_t[3, 4] = 7
    bad_order = sets.copy()
    bad_order[5] = bad_order[5][[0, 1, 2, 4, 3]]
    repeated = sets.copy()
    repeated[2, 1] = repeated[2, 0]
    long_starts = np.arange(4098, dtype=np.int64)                    # B = 4097 (and past S)
    for args, word in [((bad_t, good), b"index >= T"), ((bad_order, good), b"not strictly ascending"),
                       ((repeated, good), b"not strictly ascending"),
                       ((sets, good, 0), b"B=0"), ((sets, long_starts), b"B=4097"),
                       ((sets, [0, 50, 50, 130]), b"not above"), ((sets, [0, 60, 50, 130]), b"not above"),
                       ((sets, [-1, 50, 130]), b"negative"), ((sets, [0, 50, S + 1]), b"past the S=")]:
        rc, untouched, msg = host(*args)
        assert rc == -1 and untouched and word in msg, (word, msg)
    # the row check is one function for every width and kind of set: its two texts in full, five numbers to a row here
    assert host(bad_t, good)[2] == b"tq_patterns_quintet_blocks: row 3 has an index >= T=7"
    assert host(bad_order, good)[2] == b"tq_patterns_quintet_blocks: row 5 (0, 1, 2, 6, 5) is not strictly ascending"
    assert host(repeated, good)[2] == b"tq_patterns_quintet_blocks: row 2 (0, 0, 2, 3, 6) is not strictly ascending"
    assert lib.tq_patterns_quintet_blocks(h, None, 0, p(good), 2, None) == 0                     # Q = 0 is valid
    assert lib.tq_patterns_quintet_blocks(h, None, 0, None, 2, None) == -1
    assert lib.tq_patterns_quintet_blocks(h, None, -1, p(good), 2, None) == -1
    assert lib.tq_patterns_quintet_blocks(None, None, 0, p(good), 2, None) == -1
    with pytest.raises(ValueError):
        engine.patterns_quintet_blocks(sets[:, :4], good)
    with QuartetEngine(0) as fresh:                                                             # no data
        with pytest.raises(TetradHipError, match="TQ_ERR_NO_DATA"):
            fresh.patterns_quintet_blocks(sets, good)
    # the device form: a taxon >= T gives zero rows, everything else is refused before anything is launched
    d_sets = torch.from_numpy(bad_t.view(np.int32)).cuda()
    d_out = torch.full((len(sets), 2, 16), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    engine.patterns_quintet_blocks_dev(d_sets.data_ptr(), len(sets), good, d_out.data_ptr(), cs)
    out = d_out.cpu().numpy().view(np.uint32)
    want = qm.block_rows(g["tmparr"], sets, good)
    want[3] = 0
    assert np.array_equal(out, want)
    # a set row needs 4-byte alignment only: the rows from the second one on
    d_out.fill_(-1)
    engine.patterns_quintet_blocks_dev(d_sets.data_ptr() + 20, len(sets) - 1, good, d_out.data_ptr(), cs)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:-1], want[1:]) and (out[-1] == 0xFFFFFFFF).all()
    d_out.fill_(-1)
    for kwargs in (dict(block_starts=[0, 50, 50, 130]), dict(block_starts=[0, 50, S + 1]), dict(block_starts=[-1, 5]),
                   dict(block_starts=long_starts), dict(d_sets5=d_sets.data_ptr() + 2), dict(d_classes=d_out.data_ptr() + 8)):
        a = dict(d_sets5=d_sets.data_ptr(), Q=len(sets), block_starts=good, d_classes=d_out.data_ptr(), stream=cs)
        a.update(kwargs)
        with pytest.raises(TetradHipError, match="TQ_ERR_INVALID_ARG"):
            engine.patterns_quintet_blocks_dev(**a)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()


# ---- the device jackknife ----

@pytest.mark.parametrize("B", [1, 2, 3, 50, 4096])
def test_device_jackknife(engine, B):
    import torch
    from tetrad_amd import quintets
    N = 65 if B == 4096 else 1000
    rows, set_of, lmask, rmask = qm.jackknife_case(N, B)
    want = qm.jackknife_masks_model(rows, set_of, lmask, rmask)
    assert np.array_equal(bm.bits(quintets.dstat_jackknife_masks(rows, set_of, lmask, rmask)), bm.bits(want))
    # five invalid tests: their rows stay as they were
    skip = [10, 20, 30, 40, 50]
    set_of, lmask, rmask = set_of.copy(), lmask.copy(), rmask.copy()
    set_of[10] = rows.shape[0]
    lmask[20] |= 1
    rmask[30] = 0
    lmask[40] |= rmask[40]
    lmask[50] = 0
    d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
    d_set_of = torch.from_numpy(set_of.view(np.int32)).cuda()
    d_l, d_r = torch.from_numpy(lmask.view(np.int16)).cuda(), torch.from_numpy(rmask.view(np.int16)).cuda()
    d_out = torch.full((N + 1, 4), 2.5, dtype=torch.float64, device="cuda")
    engine.dstat_jackknife_masks_dev(d_rows.data_ptr(), rows.shape[0], B, d_set_of.data_ptr(), d_l.data_ptr(), d_r.data_ptr(), N,
                                     d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = d_out.cpu().numpy()
    keep = np.ones(N, bool)
    keep[skip] = False
    assert (got[:N][~keep] == 2.5).all() and (got[N] == 2.5).all()
    assert np.array_equal(bm.bits(got[:N][keep]), bm.bits(want[keep]))
    with pytest.raises(Exception, match="B="):
        engine.dstat_jackknife_masks_dev(d_rows.data_ptr(), rows.shape[0], 4097, d_set_of.data_ptr(), d_l.data_ptr(),
                                         d_r.data_ptr(), N, d_out.data_ptr(), 0)


# ---- end to end ----

_TREE = {}


def tree_reference(which):
    """tree_T12_S2000, every quintet with outgroup 11 and the other roles ascending, ten locus blocks: the model chain."""
    from tetrad_amd import patterns, quintets
    if "rows" not in _TREE:
        g = load_golden("tree_T12_S2000")
        tests = np.array([c + (11,) for c in combinations(range(11), 4)], np.int64)
        starts = patterns.locus_blocks(g["tmpmap"], 10)
        sets = np.unique(np.sort(tests, axis=1), axis=0)
        _TREE.update(tmparr=g["tmparr"], tmpmap=g["tmpmap"], tests=tests, starts=starts, sets=sets,
                     rows=qm.block_rows(g["tmparr"], sets, starts))
    if which not in _TREE:
        stats = getattr(quintets, which)
        masks = qm.masks(_TREE["tests"], stats)
        set_of = [int(np.flatnonzero((_TREE["sets"] == np.sort(t)).all(axis=1))[0]) for t in _TREE["tests"]]
        jk = [qm.jackknife_masks_model(_TREE["rows"], set_of, masks[:, s, 0], masks[:, s, 1]) for s in range(len(stats))]
        _TREE[which] = dict(stats=stats, masks=masks, set_of=np.array(set_of), jk=jk)
    return _TREE, _TREE[which]


def direct_count(tmparr, test, patterns_):
    """Sites of the five rows in role order that show one of the patterns: nothing missing, the 'A' rows equal the
    outgroup, the 'B' rows differ from it and agree with each other."""
    r = np.asarray(tmparr)[np.asarray(test, np.int64)].astype(np.int64)
    ok = (r <= 3).all(axis=0)
    total = 0
    for pat in patterns_:
        hit = ok.copy()
        bs = [i for i in range(5) if pat[i] == "B"]
        for i in range(4):
            hit &= (r[i] == r[4]) if pat[i] == "A" else (r[i] != r[4]) & (r[i] == r[bs[0]])
        total += int(hit.sum())
    return total


@pytest.mark.parametrize("chunk", [1 << 16, 100])
@pytest.mark.parametrize("which", ["DFOIL", "PARTITIONED_D"])
def test_run_quintet_jackknife_end_to_end(which, chunk):
    from tetrad_amd import quintets
    from tetrad_amd.engine import QuartetEngine
    r, w = tree_reference(which)
    tmparr, tmpmap, tests, stats = r["tmparr"], r["tmpmap"], r["tests"], w["stats"]
    assert len(tests) == 330 and len(r["sets"]) == 330 and len(r["starts"]) == 11               # chunk 100: 3 x 100 + 30 sets
    with QuartetEngine(0) as eng:
        res = quintets.run_quintet_jackknife(eng, tmparr, tmpmap, tests, stats, nblocks=10, chunk=chunk)
        again = quintets.run_quintet_jackknife(eng, None, None, tests, stats, block_starts=r["starts"], chunk=chunk,
                                               resident=True)
    assert res.dtype == quintets.result_dtype(stats) and len(res) == 330
    assert res.tobytes() == again.tobytes()
    sums = r["rows"].sum(axis=1, dtype=np.int64)[w["set_of"]]
    assert np.array_equal(res["nsites"], sums[:, 0])
    finite = 0
    for s, name in enumerate(stats.names):
        for side, field in enumerate(("left", "right")):
            want = [qm.mask_sum(sums[t], w["masks"][t, s, side]) for t in range(330)]
            assert np.array_equal(res[f"{name}_{field}"], np.array(want, np.uint64))
            assert want == [direct_count(tmparr, tests[t], stats[s][side]) for t in range(330)]
        jk = w["jk"][s]
        assert np.array_equal(bm.bits(res[f"{name}_D"]), bm.bits(jk[:, 1]))
        assert np.array_equal(res[f"{name}_jk_blocks"], jk[:, 0].astype(np.int64))
        assert np.array_equal(bm.bits(res[f"{name}_jk_mean"]), bm.bits(jk[:, 2]))
        se = [math.sqrt(v) if not math.isnan(v) else math.nan for v in jk[:, 3]]
        assert np.array_equal(bm.bits(res[f"{name}_jk_se"]), bm.bits(se))
        Z = [float(d) / e if e > 0 else math.nan for d, e in zip(jk[:, 1], se)]
        assert np.array_equal(bm.bits(res[f"{name}_Z"]), bm.bits(Z))
        finite += int(np.isfinite(res[f"{name}_Z"]).sum())
    assert finite > 200 * len(stats)                                                            # the case is not degenerate
