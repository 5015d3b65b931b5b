"""GPU: pooled five-taxon class rows of species sets per block of sites (`tq_block_rows_kernel<SpeciesQuintetRule>`, DESIGN.md
section 23) against the factored and the literal model, against the sample kernel under the identity map and against the
pooled four-species rows; the range rule at its edges; table freshness behind device-built replicates; refusals; and
`run_quintet_jackknife(species_of=...)` end to end.  Every comparison is bit-exact."""
import ctypes
import math
from itertools import combinations, permutations, product

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import quintets_model as qm
import species_quintets_model as sqm
from species_model import lineage_data, members, species_counts
from test_gpu_species_blocks import SHAPES, shape_cases, tiling

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 2, 4, 1, 3, 2), (12, 13, 1, 2, 5, 7)
CANARY = 0xABABABAB


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def all_sets5(K):
    return np.array(list(combinations(range(K), 5)), np.uint32)


_CASES, _RUNNING = {}, {}


def case(sizes, S=2500):
    """(tmparr, tmpmap, species_of, count table) for species of the given sizes: 10 % missing cells, 2 % redrawn cells,
    one sample in no species; built once."""
    key = (tuple(sizes), S)
    if key not in _CASES:
        tmparr, tmpmap, sp = lineage_data(sizes, S, seed=57 + len(_CASES), missing=0.10, p_within=0.02, left_out=1)
        _CASES[key] = (tmparr, tmpmap, sp, species_counts(tmparr, sp, len(sizes)))
    return _CASES[key]


def load(eng, sizes, S=2500):
    tmparr, tmpmap, sp, cnt = case(sizes, S)
    eng.set_data(tmparr, tmpmap)
    eng.set_species(sp, len(sizes))
    return tmparr, tmpmap, sp, cnt


def model(sizes, S, ssets, starts):
    """sqm.factored_rows on the case's count table; the running sums of a set are computed once and never changed."""
    cnt = case(sizes, S)[3]

    def running(_, sset):
        key = (tuple(sizes), S, tuple(int(k) for k in sset))
        if key not in _RUNNING:
            _RUNNING[key] = sqm.running_rows(cnt, sset)
            _RUNNING[key].setflags(write=False)
        return _RUNNING[key]

    return sqm.factored_rows(cnt, ssets, starts, running)


# -- rows against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sizes", [SMALL, LARGE], ids=["small", "large"])
def test_rows_against_the_factored_model(engine, sizes, shape):
    tmparr, tmpmap, sp, cnt = load(engine, sizes)
    starts = np.asarray(shape_cases(2500, tmpmap)[shape], np.int64)
    assert (np.diff(starts) > 0).all()
    ssets = all_sets5(6)
    rows = engine.patterns_quintet_blocks_species(ssets, starts)
    assert rows.dtype == np.uint32 and rows.shape == (6, len(starts) - 1, 16)
    assert np.array_equal(rows, model(sizes, 2500, ssets, starts))
    assert rows[:, :, 0].any()
    assert np.array_equal(rows[:, :, 0].astype(np.int64), rows[:, :, 1:].sum(axis=2, dtype=np.int64))


def test_4096_one_site_blocks(engine):
    load(engine, SMALL, 4100)
    starts = np.arange(2, 4099, dtype=np.int64)
    assert len(starts) - 1 == 4096
    ssets = all_sets5(6)
    assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, starts), model(SMALL, 4100, ssets, starts))
    with pytest.raises(Exception, match="B=4097"):
        engine.patterns_quintet_blocks_species(ssets, np.arange(2, 4100, dtype=np.int64))


def test_rows_against_the_literal_model(engine):
    tmparr, tmpmap, sp, cnt = load(engine, SMALL)
    starts = shape_cases(2500, tmpmap)["B7"]
    ssets = all_sets5(6)
    assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, starts), sqm.literal_rows(tmparr, sp, 6, ssets, starts))


# -- against the existing kernels -----------------------------------------------------------------------------------------
def test_identity_map_equals_the_sample_kernel(engine):
    """Every species one sample: the new kernel against tq_quintet_blocks_kernel on all C(12,5) sets."""
    g = load_golden("tree_T12_S2000")
    sets = all_sets5(12)
    assert len(sets) == 792
    engine.set_data(g["tmparr"], g["tmpmap"])
    engine.set_species(np.arange(12, dtype=np.int32), 12)
    for starts in (tiling(2000), shape_cases(2000, g["tmpmap"])["B65"], [0, 2000]):
        want = engine.patterns_quintet_blocks(sets, starts)
        assert want[:, :, 0].any()
        assert np.array_equal(engine.patterns_quintet_blocks_species(sets, starts), want)


def test_consistent_with_the_pooled_four_species_rows(engine):
    """Two bases only; species 5 is one sample that is never missing, so its per-site total is 1.  A lineage quartet of the
    species (a, b, c, d) that shows m = its "differs from position 0" bits is, with that sample, a lineage quintet of
    slot m (the sample holds position 0's base) or m | 8 (it holds the other): the pooled quartet class of m is slot m
    plus slot m | 8.  The pooled quartet rows zero class 0000, so its counterpart is read off the count table: the
    invariant lineage quartets are slot 8 plus the invariant lineage quintets."""
    from tetrad_amd import patterns
    sizes, S = (3, 2, 4, 1, 3, 1), 2500
    tmparr, tmpmap, sp = lineage_data(sizes, S, seed=91, missing=0.10, p_within=0.05, left_out=1)
    rng = np.random.default_rng(91)
    tmparr = np.where(tmparr <= 3, tmparr & 1, tmparr).astype(np.uint8)
    lone = int(np.flatnonzero(sp == 5)[0])
    gaps = tmparr[lone] > 3
    tmparr[lone, gaps] = rng.integers(0, 2, size=int(gaps.sum()), dtype=np.uint8)
    cnt = species_counts(tmparr, sp, 6)
    assert (cnt[5].sum(axis=1) == 1).all() and (tmparr > 3).any()
    sets4 = np.array(list(combinations(range(5), 4)), np.uint32)
    sets5 = np.concatenate([sets4, np.full((len(sets4), 1), 5, np.uint32)], axis=1)
    starts = shape_cases(S, tmpmap)["B7"]
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, 6)
    four = engine.patterns_blocks_species(sets4, starts)
    five = engine.patterns_quintet_blocks_species(sets5, starts)
    assert np.array_equal(five, sqm.factored_rows(cnt, sets5, starts))
    assert (five[:, :, 1:].sum(axis=1) > 0).any(axis=0).all()                  # every slot is met by some set
    for m in range(1, 8):
        cls = patterns.CLASS_STRINGS.index("0" + "".join(str((m >> i) & 1) for i in range(3)))
        assert np.array_equal(four[:, :, cls], five[:, :, m] + five[:, :, m | 8]), m
    assert np.array_equal(four[:, :, 15], five[:, :, 0] - five[:, :, 8])
    for r, (a, b, c, d) in enumerate(sets4.astype(np.int64)):
        inv4 = (cnt[a] * cnt[b] * cnt[c] * cnt[d]).sum(axis=1)                 # per site: lineage quartets on one base
        inv5 = (cnt[a] * cnt[b] * cnt[c] * cnt[d] * cnt[5]).sum(axis=1)
        for j in range(7):
            s0, s1 = int(starts[j]), int(starts[j + 1])
            assert int(five[r, j, 8]) + int(inv5[s0:s1].sum()) == int(inv4[s0:s1].sum())


# -- row counts and extremes ----------------------------------------------------------------------------------------------
NINE = (2, 1, 3, 1, 2, 1, 2, 1, 2)
STARTS3 = np.array([2, 70, 200, 257], np.int64)


@pytest.mark.parametrize("Q", [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_with_a_canary(engine, Q):
    """Sixteen lanes per item, four items per wavefront, sixteen per workgroup; B = 3 makes Q B odd for odd Q."""
    import torch
    load(engine, NINE, 257)
    ssets = all_sets5(9)[:Q]
    want = model(NINE, 257, ssets, STARTS3)
    assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, STARTS3), want)
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((Q * 3 + 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), Q, STARTS3, d_out.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:Q * 3].reshape(Q, 3, 16), want) and (out[Q * 3:] == 0xFFFFFFFF).all()


def test_host_form_chunks_by_batch(engine):
    load(engine, NINE, 257)
    ssets = all_sets5(9)
    want = model(NINE, 257, ssets, STARTS3)
    for batch in (100, 2):                                           # chunks of 33 sets; B above batch: one set a chunk
        engine.set_option("batch", batch)
        try:
            assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, STARTS3), want)
        finally:
            engine.set_option("batch", 0)


def test_device_form_bad_id_unaligned_sets_and_misaligned_rows(engine):
    """An id >= K gives a zero row; a row that repeats a species is the caller's business and follows the same formula; the
    sets may start at any dword; the rows must start at a 16-byte boundary."""
    import torch
    from tetrad_amd._lib import TetradHipError
    tmparr, tmpmap, sp, cnt = load(engine, NINE, 257)
    ssets = all_sets5(9)[:6].copy()
    ssets[2, 4] = 9
    ssets[4] = [5, 0, 0, 2, 7]
    want = sqm.factored_rows(cnt, np.where(ssets < 9, ssets, 0), STARTS3)
    want[2] = 0
    cs = torch.cuda.current_stream().cuda_stream
    for shift in (0, 1, 2, 3):                                       # dwords in front of the first row
        d_sets = torch.zeros(6 * 5 + 3, dtype=torch.int32, device="cuda")
        d_sets[shift:shift + 30] = torch.from_numpy(ssets.view(np.int32).reshape(-1)).cuda()
        d_out = torch.full((6, 3, 16), -1, dtype=torch.int32, device="cuda")
        engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr() + 4 * shift, 6, STARTS3, d_out.data_ptr(), cs)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want), shift
    d_out = torch.full((7, 3, 16), -1, dtype=torch.int32, device="cuda")
    for off in (4, 8, 12):
        with pytest.raises(TetradHipError, match="16-byte aligned"):
            engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), 6, STARTS3, d_out.data_ptr() + off, cs)
    with pytest.raises(TetradHipError, match="4-byte"):
        engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr() + 2, 6, STARTS3, d_out.data_ptr(), cs)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()


def test_device_form_row_beyond_the_range_rule(engine):
    """The host checks the range rule on the five largest species; a device row that repeats the large one can exceed it and
    gets zeros instead of counts wrapped modulo 2^32: S x 90^4 >= 2^32, and 90^5 >= 2^32 by itself."""
    import torch
    sizes, S = (90, 1, 2, 1, 1), 2000
    assert S * 90**3 * 2 < 2**32 <= S * 90**4 and 90**5 >= 2**32
    tmparr, tmpmap, sp, cnt = load(engine, sizes, S)
    ssets = np.array([[0, 1, 2, 3, 4], [0, 0, 0, 0, 1], [0, 0, 0, 2, 3], [0, 0, 0, 0, 0], [0, 2, 0, 4, 0]], np.uint32)
    starts = np.array([0, 700, S], np.int64)
    want = sqm.factored_rows(cnt, ssets[[0, 0, 2, 0, 4]], starts)
    want[1] = want[3] = 0
    assert want[[0, 2, 4], :, 0].all()
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((5, 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), 5, starts, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


def host_call(eng, ssets, starts, B=None):
    """The raw host form on canary-filled output: (rc, output untouched, message)."""
    ssets = np.ascontiguousarray(ssets, np.uint32)
    st = np.ascontiguousarray(starts, np.int64)
    nb = len(st) - 1 if B is None else B
    out = np.full((len(ssets), max(nb, 1), 16), CANARY, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = eng._lib.tq_patterns_quintet_blocks_species(eng._h, p(ssets), len(ssets), p(st), nb, p(out))
    return rc, bool((out == CANARY).all()), eng._lib.tq_last_error(eng._h)


@pytest.mark.parametrize("S", [1, 2])
def test_four_species_of_255_and_one_of_1(engine, S):
    """255^4 = 4 228 250 625 fits u32 with bit 31 set and the range rule admits one site only: at S = 2 the call is
    refused (2 x 255^4 >= 2^32) and writes nothing."""
    base = np.array([[1, 0], [1, 0], [3, 2], [1, 0], [1, 0]], np.uint8)[:, :S]           # species 2 is the one of 1
    tmparr = np.repeat(base, [255, 255, 1, 255, 255], axis=0)
    tmpmap = np.stack([np.arange(S), np.arange(S)], axis=1).astype(np.uint32)
    sp = np.repeat(np.arange(5, dtype=np.int32), [255, 255, 1, 255, 255])
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, 5)
    ssets = np.array([[0, 1, 2, 3, 4]], np.uint32)
    starts = np.arange(S + 1, dtype=np.int64)
    if S == 1:
        rows = engine.patterns_quintet_blocks_species(ssets, starts)
        want = np.zeros((1, 1, 16), np.uint32)
        want[0, 0, 2] = want[0, 0, 0] = 255**4                                           # position 2 alone differs
        assert np.array_equal(rows, want) and rows[0, 0, 2] >= 2**31
    else:
        rc, untouched, msg = host_call(engine, ssets, starts)
        assert rc == -1 and untouched and b"may exceed u32" in msg


def test_edge_of_the_five_species_range_rule(engine):
    """Five species of 11 at S = 26 668: 11^5 S = 4 294 908 068 < 2^32.  Every species is 11 copies of one sequence, so a
    row is 11^5 times the sample row of the five sequences; one block holds nearly everything and its counts have bit 31
    set.  One site more (4 295 069 119) is refused by the five-species rule."""
    S = 26668
    assert 11**5 * S == 4294908068 < 2**32 <= 11**5 * (S + 1) == 4295069119
    rng = np.random.default_rng(4)
    base = rng.integers(0, 4, size=(5, S + 1)).astype(np.uint8)
    base[:, rng.random(S + 1) < 0.6] = np.array([0, 0, 1, 1, 0], np.uint8)[:, None]     # class 2 + 4 = 6
    tmparr, sp = np.repeat(base, 11, axis=0), np.repeat(np.arange(5, dtype=np.int32), 11)
    tmpmap = np.stack([np.arange(S + 1) // 8, np.arange(S + 1)], axis=1).astype(np.uint32)
    ssets = np.array([[0, 1, 2, 3, 4]], np.uint32)
    starts = np.array([0, 1000, 2001, S], np.int64)
    engine.set_data(np.ascontiguousarray(tmparr[:, :S]), tmpmap[:S])
    engine.set_species(sp, 5)
    rows = engine.patterns_quintet_blocks_species(ssets, starts)
    want = qm.block_rows(base[:, :S], ssets, starts).astype(np.int64) * 11**5
    assert want.max() < 2**32 and np.array_equal(rows, want.astype(np.uint32))
    assert rows[0, 2, 6] >= 2**31 and rows[0, 2, 0] >= 2**31
    # the first two blocks are small enough for the factored model
    cnt = species_counts(tmparr[:, :2001], sp, 5)
    assert np.array_equal(rows[:, :2], sqm.factored_rows(cnt, ssets, starts[:3]))
    engine.set_data(tmparr, tmpmap)
    rc, untouched, msg = host_call(engine, ssets, starts)
    assert rc == -1 and untouched and b"may exceed u32" in msg and b"five largest species sizes 161051" in msg
    assert engine.patterns_blocks_species(ssets[:, :4], starts)[:, :, 15].all()            # the rule of four still holds


# -- ordering and table freshness -------------------------------------------------------------------------------------------
def test_table_follows_a_device_built_replicate():
    """bootstrap, then the call with no set_species in between: the species table is rebuilt from the new replicate."""
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    sp = np.array([0, 1, 2, 3, 4, 5, 2], np.int32)
    ssets = all_sets5(6)
    rng = np.random.default_rng(3)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        bootstrap.identity_replicate(eng)
        eng.set_species(sp, 6)
        for pack in (0, 1):
            eng.set_option("boot_pack", pack)
            seen = []
            for _ in range(2):
                S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))
                starts = tiling(S)
                rows = eng.patterns_quintet_blocks_species(ssets, starts)   # first species call behind the replicate
                tmparr, tmpmap = eng.get_data()
                assert tmparr.shape[1] == S
                assert np.array_equal(rows, sqm.factored_rows_of(tmparr, sp, 6, ssets, starts))
                lb = patterns.locus_blocks(tmpmap, 9)
                assert np.array_equal(eng.patterns_quintet_blocks_species(ssets, lb),
                                      sqm.factored_rows_of(tmparr, sp, 6, ssets, lb))
                seen.append(rows.sum(axis=1, dtype=np.uint64).tobytes())
            assert seen[0] != seen[1]                                        # the replicates differ, and so do the rows
            with pytest.raises(Exception, match="past the S="):
                eng.patterns_quintet_blocks_species(ssets, [0, S + 1])


def test_allele_mode_reads_the_source():
    """species_alleles = 1: the table comes from both alleles of the IUPAC source through the replicate's site map."""
    from species_alleles_model import haplotypes, replicate_columns
    from tetrad_amd.engine import QuartetEngine
    rng = np.random.default_rng(8)
    T, S0, K = 11, 400, 6
    seqarr = np.array([65, 67, 71, 84], np.uint8)[rng.integers(0, 4, size=(T, S0))]
    seqarr[:, ::3] = seqarr[0, ::3]                                          # shared bases, so that biallelic sites occur
    seqarr[:, 1::3] = np.where(rng.random((T, len(range(1, S0, 3)))) < 0.5, seqarr[0, 1::3], seqarr[1, 1::3])
    amb = rng.random(seqarr.shape) < 0.2
    seqarr[amb] = rng.choice(np.array([82, 75, 83, 89, 87, 77], np.uint8), size=int(amb.sum()))
    seqarr[rng.random(seqarr.shape) < 0.1] = 78
    widths = []
    while sum(widths) < S0:
        widths.append(int(min(rng.integers(1, 12), S0 - sum(widths))))
    ends = np.cumsum(widths)
    spans = np.stack([ends - widths, ends], axis=1).astype(np.int64)
    sp = np.array([0, 1, 2, 3, 4, 0, 1, 2, 5, -1, 3], np.int32)
    ssets = all_sets5(K)
    with QuartetEngine(0) as eng:
        eng.set_source(seqarr, spans)
        lidxs = rng.integers(0, len(spans), len(spans))
        S = eng.bootstrap(lidxs, 5, 6)
        eng.set_species(sp, K)
        eng.set_option("species_alleles", 1)
        cols = replicate_columns(spans, lidxs)
        assert len(cols) == S
        cnt = species_counts(np.ascontiguousarray(haplotypes(seqarr)[:, cols]), np.repeat(sp, 2), K)
        # the replicate shuffles the sites inside a locus (the model's columns are unshuffled), so the blocks are cut at
        # the replicate's locus boundaries, where a block's set of sites does not depend on that order
        bounds = np.concatenate([[0], np.cumsum((spans[:, 1] - spans[:, 0])[lidxs])])
        starts = np.unique(np.concatenate([bounds[:12], bounds[12::4], [S]]))
        assert len(starts) > 20 and starts[0] == 0 and starts[-1] == S
        rows = eng.patterns_quintet_blocks_species(ssets, starts)
        assert np.array_equal(rows, sqm.factored_rows(cnt, ssets, starts)) and rows[:, :, 0].any()
        eng.set_option("species_alleles", 0)                                 # back to one lineage per sample: other rows
        tmparr, _ = eng.get_data()
        for st in (starts, tiling(S)):                                       # the resident rows are in replicate order
            assert np.array_equal(eng.patterns_quintet_blocks_species(ssets, st), sqm.factored_rows_of(tmparr, sp, K, ssets, st))


def test_two_calls_on_another_stream(engine):
    import torch
    load(engine, SMALL)
    ssets = all_sets5(6)
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    first, second = tiling(2500), np.array([10, 50, 2390], np.int64)
    d_a = torch.zeros((6, len(first) - 1, 16), dtype=torch.int32, device="cuda")
    d_b = torch.zeros((6, 2, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    # the second call overwrites the boundaries of the first: stream order keeps the first call's kernel in front
    engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), 6, first, d_a.data_ptr(), side.cuda_stream)
    engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), 6, second, d_b.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), model(SMALL, 2500, ssets, first))
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), model(SMALL, 2500, ssets, second))


# -- refusals and options without a say --------------------------------------------------------------------------------------
def test_refusals(engine):
    import torch
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap, sp, cnt = case(SMALL)
    S = 2500
    ssets = all_sets5(6)
    good = np.array([0, 50, S], np.int64)
    with QuartetEngine(0) as fresh:
        rc, untouched, msg = host_call(fresh, ssets, good)                                 # no data
        assert rc == -4 and untouched and b"tq_set_data has not been called" in msg
        fresh.set_data(tmparr, tmpmap)
        rc, untouched, msg = host_call(fresh, ssets, good)                                 # no map
        assert rc == -4 and untouched and b"no species map" in msg
        fresh.set_species(sp, 6)
        assert host_call(fresh, ssets, good)[0] == 0
        fresh.set_data(np.ascontiguousarray(tmparr[:-2]), tmpmap)                          # a map for another T
        rc, untouched, msg = host_call(fresh, ssets, good)
        assert rc == -1 and untouched and b"the species map covers T=" in msg
        fresh.set_data(tmparr, tmpmap)
        fresh.set_option("species_alleles", 1)                                             # allele mode without a replicate
        rc, untouched, msg = host_call(fresh, ssets, good)
        assert rc == -4 and untouched and b"species_alleles needs" in msg
    load(engine, SMALL)
    assert host_call(engine, ssets, good)[:2] == (0, False)
    bad_k = ssets.copy()
    bad_k[3, 4] = 6
    bad_order = ssets.copy()
    bad_order[2] = bad_order[2][[0, 2, 1, 3, 4]]
    repeated = ssets.copy()
    repeated[1, 1] = repeated[1, 0]
    long_starts = np.arange(4098, dtype=np.int64)                                          # B = 4097 (and past S)
    for args, word in [((bad_k, good), b"index >= K"), ((bad_order, good), b"not strictly ascending"),
                       ((repeated, good), b"not strictly ascending"),
                       ((ssets, good, 0), b"B=0"), ((ssets, long_starts), b"B=4097"),
                       ((ssets, [0, 50, 50, S]), b"not above"), ((ssets, [0, 60, 50, S]), b"not above"),
                       ((ssets, [-1, 50, S]), b"negative"), ((ssets, [0, 50, S + 1]), b"past the S=")]:
        rc, untouched, msg = host_call(engine, *args)
        assert rc == -1 and untouched and word in msg and b"tq_patterns_quintet_blocks_species" in msg, (word, msg)
    assert host_call(engine, bad_k, good)[2] == b"tq_patterns_quintet_blocks_species: row 3 has an index >= K=6"
    assert host_call(engine, bad_order, good)[2] == \
        b"tq_patterns_quintet_blocks_species: row 2 (0, 2, 1, 4, 5) is not strictly ascending"
    lib, h = engine._lib, engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.tq_patterns_quintet_blocks_species(h, None, 0, p(good), 2, None) == 0       # Q = 0 is valid
    assert lib.tq_patterns_quintet_blocks_species(h, None, 0, None, 2, None) == -1
    assert lib.tq_patterns_quintet_blocks_species(h, None, -1, p(good), 2, None) == -1
    assert lib.tq_patterns_quintet_blocks_species(h, p(ssets), 6, p(good), 2, None) == -1
    assert lib.tq_patterns_quintet_blocks_species(None, None, 0, p(good), 2, None) == -1
    # the device form: everything is refused before anything is launched
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((6, 2, 16), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    for kwargs in (dict(block_starts=[0, 50, 50, S]), dict(block_starts=[0, 50, S + 1]), dict(block_starts=[-1, 5]),
                   dict(block_starts=long_starts), dict(d_ssets5=d_sets.data_ptr() + 2), dict(d_classes=d_out.data_ptr() + 8)):
        a = dict(d_ssets5=d_sets.data_ptr(), Q=6, block_starts=good, d_classes=d_out.data_ptr(), stream=cs)
        a.update(kwargs)
        with pytest.raises(TetradHipError, match="TQ_ERR_INVALID_ARG"):
            engine.patterns_quintet_blocks_species_dev(**a)
    assert lib.tq_patterns_quintet_blocks_species_dev(h, None, 6, p(good), 2, ctypes.c_void_p(d_out.data_ptr()), None) == -1
    assert lib.tq_patterns_quintet_blocks_species_dev(h, None, 0, p(good), 2, None, None) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()
    engine.patterns_quintet_blocks_species_dev(d_sets.data_ptr(), 6, good, d_out.data_ptr(), cs)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), model(SMALL, 2500, ssets, good))


def test_scan_options_and_the_locus_column_have_no_say(engine):
    tmparr, tmpmap, sp, cnt = case(SMALL)
    ssets = all_sets5(6)
    starts = tiling(2500)
    want = model(SMALL, 2500, ssets, starts)
    locus = (np.arange(2500) % 3).astype(np.uint32)                                        # an id in many runs
    engine.set_data(tmparr, locus)
    engine.set_species(sp, 6)
    with pytest.raises(Exception, match="TQ_ERR_LOCUS_ORDER"):
        engine.patterns(ssets[:, :4], True)
    assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, starts), want)
    engine.set_option("scan_method", 2)                                                    # a timing-diagnostic mode of the scans
    try:
        with pytest.raises(Exception, match="diagnostic"):
            engine.patterns_species(ssets[:, :4])
        assert np.array_equal(engine.patterns_quintet_blocks_species(ssets, starts), want)
    finally:
        engine.set_option("scan_method", -1)
    engine.timing_enable(True)
    try:
        engine.timing_read()
        engine.patterns_quintet_blocks_species(ssets, starts)
        assert engine.timing_read()[1] == 0                                                # no call was recorded
    finally:
        engine.timing_enable(False)


# -- end to end -----------------------------------------------------------------------------------------------------------------
_E2E = {}


def e2e_reference(which):
    """Six species, every role order of every set with species 5 as O, ten locus blocks: the model chain, once."""
    from tetrad_amd import patterns, quintets
    if "rows" not in _E2E:
        tmparr, tmpmap, sp = lineage_data((3, 2, 4, 1, 3, 2), 2000, 12, missing=0.1, p_within=0.05)
        tests = np.array([p + (5,) for c in combinations(range(5), 4) for p in permutations(c)], np.int64)
        starts = patterns.locus_blocks(tmpmap, 10)
        sets = np.unique(np.sort(tests, axis=1), axis=0)
        _E2E.update(tmparr=tmparr, tmpmap=tmpmap, sp=sp, tests=tests, starts=starts, sets=sets,
                    rows=sqm.factored_rows_of(tmparr, sp, 6, sets, starts))
    if which not in _E2E:
        stats = getattr(quintets, which)
        masks = qm.masks(_E2E["tests"], stats)
        set_of = [int(np.flatnonzero((_E2E["sets"] == np.sort(t)).all(axis=1))[0]) for t in _E2E["tests"]]
        jk = [qm.jackknife_masks_model(_E2E["rows"], set_of, masks[:, s, 0], masks[:, s, 1]) for s in range(len(stats))]
        _E2E[which] = dict(stats=stats, masks=masks, set_of=np.array(set_of), jk=jk)
    return _E2E, _E2E[which]


def direct_pooled_count(tmparr, sp, test, patterns_):
    """Lineage quintets (one lineage per species of `test`, in role order) times sites that show one of the patterns:
    nothing missing, the 'A' rows equal the outgroup, the 'B' rows differ from it and agree with each other."""
    mem = members(sp, 6)
    total = 0
    for lin in product(*(mem[int(k)] for k in test)):
        r = np.asarray(tmparr)[list(lin)].astype(np.int64)
        ok = (r <= 3).all(axis=0)
        for pat in patterns_:
            hit = ok.copy()
            bs = [i for i in range(5) if pat[i] == "B"]
            for i in range(4):
                hit &= (r[i] == r[4]) if pat[i] == "A" else (r[i] != r[4]) & (r[i] == r[bs[0]])
            total += int(hit.sum())
    return total


@pytest.mark.parametrize("chunk", [1 << 16, 7, 2])
@pytest.mark.parametrize("which", ["DFOIL", "PARTITIONED_D"])
def test_run_quintet_jackknife_species_end_to_end(which, chunk):
    from tetrad_amd import quintets
    from tetrad_amd.engine import QuartetEngine
    r, w = e2e_reference(which)
    tmparr, tmpmap, sp, tests, stats = r["tmparr"], r["tmpmap"], r["sp"], r["tests"], w["stats"]
    N = len(tests)
    assert N == 120 and len(r["sets"]) == 5 and len(r["starts"]) == 11                     # chunk 2: 2 + 2 + 1 sets
    with QuartetEngine(0) as eng:
        res = quintets.run_quintet_jackknife(eng, tmparr, tmpmap, tests, stats, nblocks=10, chunk=chunk, species_of=sp)
        again = quintets.run_quintet_jackknife(eng, None, None, tests, stats, block_starts=r["starts"], chunk=chunk,
                                               resident=True, species_of=sp)
    assert res.dtype == quintets.result_dtype(stats) and len(res) == N
    assert res.tobytes() == again.tobytes()
    sums = r["rows"].sum(axis=1, dtype=np.int64)[w["set_of"]]
    assert np.array_equal(res["nsites"], sums[:, 0])
    finite = 0
    for s, name in enumerate(stats.names):
        for side, field in enumerate(("left", "right")):
            want = [qm.mask_sum(sums[t], w["masks"][t, s, side]) for t in range(N)]
            assert np.array_equal(res[f"{name}_{field}"], np.array(want, np.uint64))
            if chunk == 7:                                                                 # once per statistic: a test in 13
                for t in range(s, N, 13):
                    assert want[t] == direct_pooled_count(tmparr, sp, tests[t], stats[s][side])
        jk = w["jk"][s]
        assert np.array_equal(bm.bits(res[f"{name}_D"]), bm.bits(jk[:, 1]))
        assert np.array_equal(res[f"{name}_jk_blocks"], jk[:, 0].astype(np.int64))
        assert np.array_equal(bm.bits(res[f"{name}_jk_mean"]), bm.bits(jk[:, 2]))
        se = [math.sqrt(v) if not math.isnan(v) else math.nan for v in jk[:, 3]]
        assert np.array_equal(bm.bits(res[f"{name}_jk_se"]), bm.bits(se))
        Z = [float(d) / e if e > 0 else math.nan for d, e in zip(jk[:, 1], se)]
        assert np.array_equal(bm.bits(res[f"{name}_Z"]), bm.bits(Z))
        finite += int(np.isfinite(res[f"{name}_Z"]).sum())
    assert finite > 80 * len(stats)                                                        # the case is not degenerate
