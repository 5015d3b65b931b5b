"""CPU-only: the pooled five-taxon rule of species block rows.  The two routes of the model agree,
and `tq_pooled_quintet_site_classes` -- the host execution of the functions the kernel runs per site, products of
multi-dots minus the quintuple dot -- equals plain enumeration of the 1024 patterns."""
import ctypes
import inspect
from itertools import combinations, product

import numpy as np
import pytest

import quintets_model as qm
import species_quintets_model as sqm
from species_blocks_model import pack_counts
from species_model import lineage_data

CANARY = 0xABABABAB


@pytest.fixture(scope="module")
def lib():
    from tetrad_amd import _lib
    _lib.build()
    return _lib.load()


def pooled(lib, counts5) -> np.ndarray:
    """tq_pooled_quintet_site_classes on counts [5 species, 4 bases] -> u32[16]"""
    packed = np.ascontiguousarray(pack_counts(counts5))
    assert packed.shape == (5,)
    out = np.full(16, CANARY, np.uint32)
    rc = lib.tq_pooled_quintet_site_classes(packed.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def check(lib, counts5):
    """The library's row equals the enumeration (which must fit u32) and slot 0 is the sum of slots 1..15."""
    want = sqm.site_row(counts5)
    assert want.max() < 2**32
    got = pooled(lib, counts5).astype(np.int64)
    assert np.array_equal(got, want), (np.asarray(counts5).tolist(), got, want)
    assert got[0] == got[1:].sum()
    return got


# -- the two routes of the model ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    sizes = (1, 2, 3, 4, 6, 2)
    tmparr, tmpmap, sp = lineage_data(sizes, 130, seed=5, missing=0.15, p_within=0.1, left_out=1)
    assert tmparr.shape == (19, 130) and (sp == -1).sum() == 1
    return tmparr, sp, np.array(list(combinations(range(6), 5)), np.uint32)


@pytest.mark.parametrize("starts", [[0, 130], [0, 15, 16, 17, 100, 130], list(range(40, 60))], ids=["B1", "B5", "one_site"])
def test_literal_and_factored_routes_agree(case, starts):
    tmparr, sp, ssets = case
    lit = sqm.literal_rows(tmparr, sp, 6, ssets, starts)
    fac = sqm.factored_rows_of(tmparr, sp, 6, ssets, starts)
    assert lit.shape == (6, len(starts) - 1, 16)
    assert np.array_equal(lit, fac)
    assert np.array_equal(lit[:, :, 0].astype(np.int64), lit[:, :, 1:].sum(axis=2, dtype=np.int64))
    assert lit[:, :, 0].any()


def test_class_table_of_the_model_is_the_library_s(lib):
    out = np.zeros(1024, np.uint8)
    assert lib.tq_quintet_class_table(out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(out, qm.class_table())


# -- the library's rule against enumeration ---------------------------------------------------------------------------------
def random_counts(rng):
    """Five species of random sizes whose product stays below 2^32, each spread over the bases with a random share of
    its lineages missing."""
    sizes = np.exp(rng.uniform(np.log(2), np.log(256), size=5)).astype(np.int64).clip(0, 255)
    while int(np.prod(sizes)) >= 2**32:
        sizes[np.argmax(sizes)] //= 2
    counts = np.zeros((5, 4), np.int64)
    for i, n in enumerate(sizes):
        present = int(rng.integers(0, n + 1)) if rng.random() < 0.3 else int(n)
        counts[i] = rng.multinomial(present, rng.dirichlet(np.full(4, 0.4)))
    return counts


def test_random_count_quintuples(lib):
    rng = np.random.default_rng(23)
    nonzero = big = 0
    for _ in range(2000):
        got = check(lib, random_counts(rng))
        nonzero += int(got[0] > 0)
        big += int(got.max() >= 2**24)
    assert nonzero > 1000 and big > 100                 # the draw reaches counted sites and products beyond 24 bits


def test_all_zero_and_an_all_missing_species(lib):
    assert not check(lib, np.zeros((5, 4), np.int64)).any()
    full = np.array([[3, 1, 0, 2], [0, 4, 4, 0], [7, 0, 1, 0], [2, 2, 2, 2], [1, 0, 0, 5]], np.int64)
    assert check(lib, full)[0] > 0
    for i in range(5):
        c = full.copy()
        c[i] = 0
        assert not check(lib, c).any()


def test_all_1024_unit_patterns(lib):
    cls = qm.class_table()
    per_class = np.zeros(16, np.int64)
    for p, x in enumerate(product(range(4), repeat=5)):
        c = np.zeros((5, 4), np.int64)
        c[np.arange(5), x] = 1
        want = np.zeros(16, np.int64)
        if cls[p]:
            want[cls[p]] = want[0] = 1
        assert np.array_equal(pooled(lib, c).astype(np.int64), want), x
        per_class[cls[p]] += 1
    assert per_class[0] == 1024 - 180 and (per_class[1:] == 12).all()


def test_five_species_on_one_base(lib):
    for base in range(4):
        c = np.zeros((5, 4), np.int64)
        c[:, base] = [255, 255, 255, 255, 1]
        assert not check(lib, c).any()
        c[:, base] = [9, 200, 31, 1, 77]
        assert not check(lib, c).any()


@pytest.mark.parametrize("odd", range(5))
def test_four_species_of_255_and_one_lineage_apart(lib, odd):
    """255^4 = 4 228 250 625 in one slot, bit 31 set: the quadruple dot of the four agreeing species times the total of
    the fifth, for the odd species in each position."""
    c = np.zeros((5, 4), np.int64)
    c[:, 1] = 255
    c[odd] = [0, 0, 0, 1]
    got = check(lib, c)
    slot = 15 if odd == 0 else 1 << (odd - 1)
    want = np.zeros(16, np.int64)
    want[slot] = want[0] = 255**4
    assert np.array_equal(got, want) and got[slot] >= 2**31


@pytest.mark.parametrize("odd", range(5))
def test_a_quadruple_dot_beyond_24_bits(lib, odd):
    """255 lineages spread over two bases: the quadruple dot 128^4 + 127^4 does not fit the 24-bit multiplier."""
    assert 128**4 + 127**4 > 2**24 and 70**4 + 30**4 > 2**24
    c = np.zeros((5, 4), np.int64)
    c[:, 0], c[:, 2] = 128, 127
    c[odd] = [1, 0, 0, 0]
    got = check(lib, c)
    assert (got[1:] > 0).all()                          # two bases everywhere: every class occurs
    c[:, 0], c[:, 2] = 70, 30
    c[odd] = [2, 0, 1, 0]
    assert check(lib, c).max() >= 2**24


def test_null_pointers_are_refused(lib):
    out = np.zeros(16, np.uint32)
    assert lib.tq_pooled_quintet_site_classes(None, out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.tq_pooled_quintet_site_classes(out.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert b"tq_pooled_quintet_site_classes" in lib.tq_last_error(None)


# -- the driver's signature -----------------------------------------------------------------------------------------------
def test_run_quintet_jackknife_signature(lib):
    """`species_of` is keyword-only with default None; every other parameter and default is what it was."""
    from tetrad_amd import quintets
    params = inspect.signature(quintets.run_quintet_jackknife).parameters
    assert list(params) == ["engine", "tmparr", "tmpmap", "tests", "stats", "nblocks", "block_starts", "chunk", "resident",
                            "species_of"]
    assert params["stats"].default is quintets.DFOIL and params["nblocks"].default == 50
    assert params["block_starts"].default is None and params["chunk"].default == 1 << 16
    for name, default in (("resident", False), ("species_of", None)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is default
