"""GPU: pooled class rows of species sets per block of sites (`tq_block_rows_kernel<SpeciesRule>`) against
the factored and the literal model, against `patterns_species` (summed over a tiling) and against the sample kernel under
the identity map; table freshness behind device-built replicates; refusals; and `run_dstat_jackknife(species_of=...)`
end to end.  Every comparison is bit-exact."""
import ctypes
import math
from itertools import combinations

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import species_blocks_model as sbm
from species_model import lineage_data, species_counts, spike_data

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 2, 11, 1, 4), (12, 13, 1, 2, 5)          # LARGE is above the bound of the MFMA pooling kernel
CANARY = 0xABABABAB


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def all_sets(K):
    return np.array(list(combinations(range(K), 4)), np.uint32)


_CASES = {}


def case(sizes, S=2500):
    """(tmparr, tmpmap, species_of, count table) for species of the given sizes: 10 % missing cells, 2 % redrawn cells,
    one sample in no species; built once."""
    key = (tuple(sizes), S)
    if key not in _CASES:
        tmparr, tmpmap, sp = lineage_data(sizes, S, seed=31 + len(_CASES), missing=0.10, p_within=0.02, left_out=1)
        _CASES[key] = (tmparr, tmpmap, sp, species_counts(tmparr, sp, len(sizes)))
    return _CASES[key]


def load(eng, sizes, S=2500):
    tmparr, tmpmap, sp, cnt = case(sizes, S)
    eng.set_data(tmparr, tmpmap)
    eng.set_species(sp, len(sizes))
    return tmparr, tmpmap, sp, cnt


def tiling(S):
    cuts = sorted({c for c in (1, 5, 15, 16, 17, 64, 100, 129, 256, 300, 1023, 1024, 1025) if c < S})
    return np.array([0] + cuts + [S], np.int64)


def shape_cases(S, tmpmap):
    """The block shapes of test_gpu_blocks.py with the cuts this kernel can trip over: a lane takes every 16th site."""
    from tetrad_amd import patterns
    return {
        "whole": [0, S],
        "one_site_blocks": list(range(90, 131)),
        "inside_16_sites": [45, 49],
        "last_sites": [S - 3, S],
        "sixteen_edges": [0, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, S],
        "many_steps_per_lane": [5, 1200, S],
        "head_and_tail_uncovered": [17, 400, 900, 2400],
        "B7": np.linspace(0, S, 8).astype(np.int64),
        "B64": np.linspace(3, S - 2, 65).astype(np.int64),
        "B65": np.linspace(0, S, 66).astype(np.int64),
        "locus_blocks": patterns.locus_blocks(tmpmap, 10),
    }


SHAPES = ["whole", "one_site_blocks", "inside_16_sites", "last_sites", "sixteen_edges", "many_steps_per_lane",
          "head_and_tail_uncovered", "B7", "B64", "B65", "locus_blocks"]


# -- rows against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sizes", [SMALL, LARGE])
def test_rows_against_the_factored_model(engine, sizes, shape):
    tmparr, tmpmap, sp, cnt = load(engine, sizes)
    starts = np.asarray(shape_cases(2500, tmpmap)[shape], np.int64)
    assert (np.diff(starts) > 0).all()
    ssets = all_sets(5)
    rows = engine.patterns_blocks_species(ssets, starts)
    assert rows.dtype == np.uint32 and rows.shape == (5, len(starts) - 1, 16)
    assert np.array_equal(rows, sbm.factored_rows(cnt, ssets, starts))
    assert rows[:, :, 15].any() and not rows[:, :, 0].any()


def test_4096_one_site_blocks(engine):
    tmparr, tmpmap, sp, cnt = load(engine, SMALL, 4100)
    starts = np.arange(2, 4099, dtype=np.int64)
    assert len(starts) - 1 == 4096
    ssets = all_sets(5)
    assert np.array_equal(engine.patterns_blocks_species(ssets, starts), sbm.factored_rows(cnt, ssets, starts))
    with pytest.raises(Exception, match="B=4097"):
        engine.patterns_blocks_species(ssets, np.arange(2, 4100, dtype=np.int64))


def test_rows_against_the_literal_model(engine):
    tmparr, tmpmap, sp, cnt = load(engine, SMALL)
    starts = shape_cases(2500, tmpmap)["B7"]
    ssets = all_sets(5)
    assert np.array_equal(engine.patterns_blocks_species(ssets, starts), sbm.literal_rows(tmparr, sp, 5, ssets, starts))


# -- against the existing paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("sizes,method", [(SMALL, 0), (SMALL, 1), (LARGE, 0)])
def test_a_tiling_sums_to_patterns_species(engine, sizes, method, inv):
    load(engine, sizes)
    ssets = all_sets(5)
    engine.set_option("species_method", method)
    engine.set_option("count_invariant", inv)
    try:
        whole = engine.patterns_species(ssets)
        rows = engine.patterns_blocks_species(ssets, tiling(2500))
        one = engine.patterns_blocks_species(ssets, [0, 2500])
    finally:
        engine.set_option("count_invariant", 0)
        engine.set_option("species_method", -1)
    assert whole[:, 15].all()
    assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), whole.astype(np.uint64))
    assert np.array_equal(one[:, 0], whole)


def test_identity_map_equals_the_sample_kernel(engine):
    """Every species one sample: the new kernel against tq_block_rows_kernel<QuartetRule> on the same sets."""
    g = load_golden("carry_T6_S2500")
    sets = all_sets(6)
    engine.set_data(g["tmparr"], g["tmpmap"])
    engine.set_species(np.arange(6, dtype=np.int32), 6)
    for starts in (tiling(2500), shape_cases(2500, g["tmpmap"])["B65"]):
        want = engine.patterns_blocks(sets, starts)
        assert want[:, :, 15].any()
        assert np.array_equal(engine.patterns_blocks_species(sets, starts), want)
        engine.set_option("count_invariant", 1)                      # the sample rows gain class 0, the pooled rows do not
        try:
            assert engine.patterns_blocks(sets, starts)[:, :, 0].any()
            assert np.array_equal(engine.patterns_blocks_species(sets, starts), want)
        finally:
            engine.set_option("count_invariant", 0)


# -- row counts and extremes ----------------------------------------------------------------------------------------------
EIGHT = (2, 1, 3, 1, 2, 1, 2, 1)
STARTS3 = np.array([2, 70, 200, 257], np.int64)


@pytest.mark.parametrize("Q", [1, 3, 4, 5, 63, 64, 65])
def test_row_counts_with_a_canary(engine, Q):
    """Sixteen lanes per item, four items per wavefront, sixteen per workgroup; B = 3 makes Q B odd for odd Q."""
    import torch
    tmparr, tmpmap, sp, cnt = load(engine, EIGHT, 257)
    ssets = all_sets(8)[:Q]
    want = sbm.factored_rows(cnt, ssets, STARTS3)
    assert np.array_equal(engine.patterns_blocks_species(ssets, STARTS3), want)
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((Q * 3 + 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), Q, STARTS3, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:Q * 3].reshape(Q, 3, 16), want) and (out[Q * 3:] == 0xFFFFFFFF).all()


def test_host_form_chunks_by_batch(engine):
    tmparr, tmpmap, sp, cnt = load(engine, EIGHT, 257)
    ssets = all_sets(8)
    want = sbm.factored_rows(cnt, ssets, STARTS3)
    for batch in (100, 2):                                           # chunks of 33 sets; B above batch: one set a chunk
        engine.set_option("batch", batch)
        try:
            assert np.array_equal(engine.patterns_blocks_species(ssets, STARTS3), want)
        finally:
            engine.set_option("batch", 0)


def test_device_form_bad_id_and_repeated_species(engine):
    """An id >= K gives a zero row; a row that repeats a species is the caller's business and follows the same formula."""
    import torch
    tmparr, tmpmap, sp, cnt = load(engine, EIGHT, 257)
    ssets = all_sets(8)[:6].copy()
    ssets[2, 3] = 8
    ssets[4] = [5, 0, 0, 2]
    want = sbm.factored_rows(cnt, np.where(ssets < 8, ssets, 0), STARTS3)
    want[2] = 0
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((6, 3, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), 6, STARTS3, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


def test_device_form_row_beyond_the_range_rule(engine):
    """The host checks the range rule on the four largest species; a device row that repeats the large one can exceed it
    (S x 40^4 >= 2^32 here) and gets zeros, as in the pooling kernels, instead of counts wrapped modulo 2^32."""
    import torch
    sizes, S = (40, 1, 2, 1), 2000
    assert S * 40 * 2 < 2**32 <= S * 40**4 and S * 40**3 * 2 < 2**32
    tmparr, tmpmap, sp, cnt = load(engine, sizes, S)
    ssets = np.array([[0, 1, 2, 3], [0, 0, 0, 0], [0, 0, 0, 2], [0, 0, 2, 0]], np.uint32)
    starts = np.array([0, 700, S], np.int64)
    want = sbm.factored_rows(cnt, ssets[[0, 0, 2, 3]], starts)
    want[1] = 0
    assert want[2:, :, 15].all()
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((4, 2, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), 4, starts, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("S", [1, 2, 3])
def test_four_species_of_255(engine, S):
    """255^4 = 4 228 250 625 fits u32 with bit 31 set, and the range rule S x 255^4 < 2^32 admits one site only: at
    S = 2 and 3 the call is refused with the message of every species call and writes nothing."""
    base = np.array([[0, 1, 0], [0, 1, 2], [1, 0, 0], [1, 0, 3]], np.uint8)[:, :S]       # site 0: AACC, site 1: CCAA
    tmparr = np.repeat(base, 255, axis=0)
    tmpmap = np.stack([np.arange(S), np.arange(S)], axis=1).astype(np.uint32)
    sp = np.repeat(np.arange(4, dtype=np.int32), 255)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, 4)
    ssets = np.array([[0, 1, 2, 3]], np.uint32)
    starts = np.arange(S + 1, dtype=np.int64)
    if S == 1:
        rows = engine.patterns_blocks_species(ssets, starts)
        want = np.zeros((1, 1, 16), np.uint32)
        want[0, 0, 3] = want[0, 0, 15] = 255**4
        assert np.array_equal(rows, want) and rows[0, 0, 3] >= 2**31
        assert np.array_equal(rows[:, 0], engine.patterns_species(ssets))
    else:
        out = np.full((1, S, 16), CANARY, np.uint32)
        rc = engine._lib.tq_patterns_blocks_species(engine._h, ctypes.c_void_p(ssets.ctypes.data), 1,
                                                    ctypes.c_void_p(starts.ctypes.data), S, ctypes.c_void_p(out.ctypes.data))
        assert rc == -1 and (out == CANARY).all() and b"may exceed u32" in engine._lib.tq_last_error(engine._h)


def test_edge_of_the_range_rule(engine):
    """Four species of 11 at S = 293 352: 11^4 S = 2^32 - 664.  One block holds nearly everything, so its counts have bit
    31 set; the blocks sum to the row of patterns_species.  One site more is refused."""
    S = 293352
    assert 11**4 * S < 2**32 <= 11**4 * (S + 1)
    tmparr, sp = spike_data(S + 1, 11)
    tmpmap = np.stack([np.arange(S + 1) // 8, np.arange(S + 1)], axis=1).astype(np.uint32)
    ssets = np.array([[0, 1, 2, 3]], np.uint32)
    starts = np.array([0, 1000, 2001, S], np.int64)
    engine.set_data(np.ascontiguousarray(tmparr[:, :S]), tmpmap[:S])
    engine.set_species(sp, 4)
    rows = engine.patterns_blocks_species(ssets, starts)
    whole = engine.patterns_species(ssets)
    assert rows[0, 2, 3] >= 2**31 and rows[0, 2, 15] >= 2**31
    assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), whole.astype(np.uint64))
    # the first two blocks are small enough for the model
    cnt = species_counts(tmparr[:, :2001], sp, 4)
    assert np.array_equal(rows[:, :2], sbm.factored_rows(cnt, ssets, starts[:3]))
    engine.set_data(tmparr, tmpmap)
    with pytest.raises(Exception, match="may exceed u32"):
        engine.patterns_blocks_species(ssets, starts)


# -- ordering and table freshness -------------------------------------------------------------------------------------------
def test_table_follows_a_device_built_replicate():
    """bootstrap, then the call with no set_species in between: the species table is rebuilt from the new replicate."""
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    sp = np.array([0, 1, 2, 3, 4, 0, 2], np.int32)
    ssets = all_sets(5)
    rng = np.random.default_rng(3)
    with QuartetEngine(0) as eng:
        eng.set_source(g["seqarr"], g["spans"])
        bootstrap.identity_replicate(eng)
        eng.set_species(sp, 5)
        for pack in (0, 1):
            eng.set_option("boot_pack", pack)
            seen = []
            for _ in range(2):
                S = eng.bootstrap(*bootstrap.draw_replicate(len(g["spans"]), rng))
                starts = tiling(S)
                rows = eng.patterns_blocks_species(ssets, starts)           # first species call behind the replicate
                tmparr, tmpmap = eng.get_data()
                assert tmparr.shape[1] == S
                assert np.array_equal(rows, sbm.factored_rows_of(tmparr, sp, 5, ssets, starts))
                lb = patterns.locus_blocks(tmpmap, 9)
                assert np.array_equal(eng.patterns_blocks_species(ssets, lb), sbm.factored_rows_of(tmparr, sp, 5, ssets, lb))
                seen.append(rows.sum(axis=1, dtype=np.uint64).tobytes())
            assert seen[0] != seen[1]                                        # the replicates differ, and so do the rows
            with pytest.raises(Exception, match="past the S="):
                eng.patterns_blocks_species(ssets, [0, S + 1])


def test_allele_mode_reads_the_source(engine):
    """species_alleles = 1: the table comes from both alleles of the IUPAC source through the replicate's site map."""
    from species_alleles_model import haplotypes, replicate_columns
    from tetrad_amd.engine import QuartetEngine
    rng = np.random.default_rng(8)
    T, S0, K = 11, 400, 5
    seqarr = np.array([65, 67, 71, 84], np.uint8)[rng.integers(0, 4, size=(T, S0))]
    seqarr[:, ::3] = seqarr[0, ::3]                                          # shared bases, so that pairs and triples occur
    amb = rng.random(seqarr.shape) < 0.2
    seqarr[amb] = rng.choice(np.array([82, 75, 83, 89, 87, 77], np.uint8), size=int(amb.sum()))
    seqarr[rng.random(seqarr.shape) < 0.1] = 78
    widths = []
    while sum(widths) < S0:
        widths.append(int(min(rng.integers(1, 12), S0 - sum(widths))))
    ends = np.cumsum(widths)
    spans = np.stack([ends - widths, ends], axis=1).astype(np.int64)
    sp = np.array([0, 1, 2, 3, 4, 0, 1, 2, 0, -1, 3], np.int32)
    ssets = all_sets(K)
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
        # the replicate's locus boundaries, where a block's set of sites does not depend on that order: eleven
        # one-locus blocks, then four loci a block
        bounds = np.concatenate([[0], np.cumsum((spans[:, 1] - spans[:, 0])[lidxs])])
        starts = np.unique(np.concatenate([bounds[:12], bounds[12::4], [S]]))
        assert len(starts) > 20 and starts[0] == 0 and starts[-1] == S
        rows = eng.patterns_blocks_species(ssets, starts)
        assert np.array_equal(rows, sbm.factored_rows(cnt, ssets, starts))
        assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), eng.patterns_species(ssets).astype(np.uint64))
        eng.set_option("species_alleles", 0)                                 # back to one lineage per sample: other rows
        tmparr, _ = eng.get_data()
        for st in (starts, tiling(S)):                                       # the resident rows are in replicate order
            assert np.array_equal(eng.patterns_blocks_species(ssets, st), sbm.factored_rows_of(tmparr, sp, K, ssets, st))


def test_two_calls_on_another_stream(engine):
    import torch
    tmparr, tmpmap, sp, cnt = load(engine, SMALL)
    ssets = all_sets(5)
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    first, second = tiling(2500), np.array([10, 50, 2390], np.int64)
    d_a = torch.zeros((5, len(first) - 1, 16), dtype=torch.int32, device="cuda")
    d_b = torch.zeros((5, 2, 16), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    # the second call overwrites the boundaries of the first: stream order keeps the first call's kernel in front
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), 5, first, d_a.data_ptr(), side.cuda_stream)
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), 5, second, d_b.data_ptr(), side.cuda_stream)
    side.synchronize()
    assert np.array_equal(d_a.cpu().numpy().view(np.uint32), sbm.factored_rows(cnt, ssets, first))
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), sbm.factored_rows(cnt, ssets, second))


# -- refusals and options without a say --------------------------------------------------------------------------------------
def host_call(eng, ssets, starts, B=None):
    """The raw host form on canary-filled output: (rc, output untouched, message)."""
    ssets = np.ascontiguousarray(ssets, np.uint32)
    st = np.ascontiguousarray(starts, np.int64)
    nb = len(st) - 1 if B is None else B
    out = np.full((len(ssets), max(nb, 1), 16), CANARY, np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = eng._lib.tq_patterns_blocks_species(eng._h, p(ssets), len(ssets), p(st), nb, p(out))
    return rc, bool((out == CANARY).all()), eng._lib.tq_last_error(eng._h)


def test_refusals(engine):
    import torch
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap, sp, cnt = case(SMALL)
    S = 2500
    ssets = all_sets(5)
    good = np.array([0, 50, S], np.int64)
    with QuartetEngine(0) as fresh:
        rc, untouched, msg = host_call(fresh, ssets, good)                                 # no data
        assert rc == -4 and untouched and b"tq_set_data has not been called" in msg
        fresh.set_data(tmparr, tmpmap)
        rc, untouched, msg = host_call(fresh, ssets, good)                                 # no map
        assert rc == -4 and untouched and b"no species map" in msg
        fresh.set_species(sp, 5)
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
    bad_k[3, 3] = 5
    bad_order = ssets.copy()
    bad_order[2] = bad_order[2][[0, 2, 1, 3]]
    long_starts = np.arange(4098, dtype=np.int64)                                          # B = 4097 (and past S)
    for args, word in [((bad_k, good), b"index >= K"), ((bad_order, good), b"not strictly ascending"),
                       ((ssets, good, 0), b"B=0"), ((ssets, long_starts), b"B=4097"),
                       ((ssets, [0, 50, 50, S]), b"not above"), ((ssets, [0, 60, 50, S]), b"not above"),
                       ((ssets, [-1, 50, S]), b"negative"), ((ssets, [0, 50, S + 1]), b"past the S=")]:
        rc, untouched, msg = host_call(engine, *args)
        assert rc == -1 and untouched and word in msg and b"tq_patterns_blocks_species" in msg, (word, msg)
    # the row check is one function for every width and kind of set: its two texts in full
    assert host_call(engine, bad_k, good)[2] == b"tq_patterns_blocks_species: row 3 has an index >= K=5"
    assert host_call(engine, bad_order, good)[2] == b"tq_patterns_blocks_species: row 2 (0, 3, 1, 4) is not strictly ascending"
    lib, h = engine._lib, engine._h
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.tq_patterns_blocks_species(h, None, 0, p(good), 2, None) == 0               # Q = 0 is valid
    assert lib.tq_patterns_blocks_species(h, None, 0, None, 2, None) == -1
    assert lib.tq_patterns_blocks_species(h, None, -1, p(good), 2, None) == -1
    assert lib.tq_patterns_blocks_species(h, p(ssets), 5, p(good), 2, None) == -1
    assert lib.tq_patterns_blocks_species(None, None, 0, p(good), 2, None) == -1
    # the device form: everything is refused before anything is launched
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_out = torch.full((5, 2, 16), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    for kwargs in (dict(block_starts=[0, 50, 50, S]), dict(block_starts=[0, 50, S + 1]), dict(block_starts=[-1, 5]),
                   dict(block_starts=long_starts), dict(d_ssets=d_sets.data_ptr() + 4), dict(d_classes=d_out.data_ptr() + 8)):
        a = dict(d_ssets=d_sets.data_ptr(), Q=5, block_starts=good, d_classes=d_out.data_ptr(), stream=cs)
        a.update(kwargs)
        with pytest.raises(TetradHipError, match="TQ_ERR_INVALID_ARG"):
            engine.patterns_blocks_species_dev(**a)
    assert lib.tq_patterns_blocks_species_dev(h, None, 5, p(good), 2, ctypes.c_void_p(d_out.data_ptr()), None) == -1
    assert lib.tq_patterns_blocks_species_dev(h, None, 0, p(good), 2, None, None) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == -1).all()
    engine.patterns_blocks_species_dev(d_sets.data_ptr(), 5, good, d_out.data_ptr(), cs)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), sbm.factored_rows(cnt, ssets, good))


def test_scan_options_and_the_locus_column_have_no_say(engine):
    tmparr, tmpmap, sp, cnt = case(SMALL)
    ssets = all_sets(5)
    starts = tiling(2500)
    want = sbm.factored_rows(cnt, ssets, starts)
    locus = (np.arange(2500) % 3).astype(np.uint32)                                        # an id in many runs
    engine.set_data(tmparr, locus)
    engine.set_species(sp, 5)
    with pytest.raises(Exception, match="TQ_ERR_LOCUS_ORDER"):
        engine.patterns(ssets, True)
    assert np.array_equal(engine.patterns_blocks_species(ssets, starts), want)
    engine.set_option("scan_method", 2)                                                    # a timing-diagnostic mode of the scans
    try:
        with pytest.raises(Exception, match="diagnostic"):
            engine.patterns_species(ssets)
        assert np.array_equal(engine.patterns_blocks_species(ssets, starts), want)
    finally:
        engine.set_option("scan_method", -1)
    engine.timing_enable(True)
    try:
        engine.timing_read()
        engine.patterns_blocks_species(ssets, starts)
        assert engine.timing_read()[1] == 0                                                # no call was recorded
    finally:
        engine.timing_enable(False)


# -- end to end -----------------------------------------------------------------------------------------------------------------
_E2E = {}


def e2e_reference():
    """Six species, every test with outgroup species 5, ten locus blocks: the model chain, once."""
    if not _E2E:
        from tetrad_amd import patterns
        tmparr, tmpmap, sp = lineage_data((3, 2, 4, 1, 3, 2), 2000, 12, missing=0.1, p_within=0.05)
        tests = patterns.tests_with_outgroup(6, 5)
        starts = patterns.locus_blocks(tmpmap, 10)
        sets, set_of, idx = patterns._role_classes(tests, (patterns.ABBA, patterns.BABA, patterns.BBAA))
        rows = sbm.factored_rows_of(tmparr, sp, 6, sets, starts)
        jk = bm.jackknife_model(rows, set_of, idx[:, 0], idx[:, 1])
        _E2E.update(tmparr=tmparr, tmpmap=tmpmap, sp=sp, tests=tests, starts=starts, sets=sets, set_of=set_of, idx=idx,
                    rows=rows, jk=jk)
    return _E2E


@pytest.mark.parametrize("chunk", [1 << 16, 7])
def test_run_dstat_jackknife_species_end_to_end(chunk):
    from tetrad_amd import patterns
    from tetrad_amd.engine import QuartetEngine
    r = e2e_reference()
    tmparr, tmpmap, sp, tests = r["tmparr"], r["tmpmap"], r["sp"], r["tests"]
    assert len(tests) == 30 and len(r["sets"]) == 10 and len(r["starts"]) >= 3            # chunk 7: 7 + 3 sets
    with QuartetEngine(0) as eng:
        res = patterns.run_dstat_jackknife(eng, tmparr, tmpmap, tests, block_starts=r["starts"], chunk=chunk, species_of=sp)
        again = patterns.run_dstat_jackknife(eng, None, None, tests, block_starts=r["starts"], chunk=chunk, resident=True,
                                             species_of=sp)
        cuts = patterns.run_dstat_jackknife(eng, tmparr, tmpmap, tests, nblocks=10, chunk=chunk, species_of=sp)
        boot = patterns.run_dstat(eng, tmparr, tmpmap, None, None, tests, 0, species_of=sp)
    assert res.dtype == patterns.JACKKNIFE_DTYPE and len(res) == 30
    assert res.tobytes() == again.tobytes() == cuts.tobytes()
    sums = r["rows"].sum(axis=1, dtype=np.int64)
    set_of, idx, jk = r["set_of"].astype(np.int64), r["idx"].astype(np.int64), r["jk"]
    assert np.array_equal(res["abba"], sums[set_of, idx[:, 0]]) and np.array_equal(res["baba"], sums[set_of, idx[:, 1]])
    assert np.array_equal(res["bbaa"], sums[set_of, idx[:, 2]]) and np.array_equal(res["nsites"], sums[set_of, 15])
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
    assert np.isfinite(res["Z"]).sum() >= 25                                               # the case is not degenerate
