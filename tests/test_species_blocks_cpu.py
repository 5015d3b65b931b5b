"""CPU-only: the pooled class rule of species block rows.  The two routes of the model agree, and
`tq_pooled_site_classes` -- the host execution of the function the kernel runs per site, partition sums and their
Moebius inversion -- equals plain enumeration of the 256 patterns."""
import ctypes

import numpy as np
import pytest

import species_blocks_model as sbm
from species_model import lineage_data

SIZES = (1, 2, 3, 4, 6)


@pytest.fixture(scope="module")
def lib():
    from tetrad_amd import _lib
    _lib.build()
    return _lib.load()


def pooled(lib, counts4) -> np.ndarray:
    """tq_pooled_site_classes on counts [4 species, 4 bases] -> u32[16]"""
    packed = np.ascontiguousarray(sbm.pack_counts(counts4))
    out = np.full(16, 0xABABABAB, np.uint32)
    rc = lib.tq_pooled_site_classes(packed.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def case():
    tmparr, tmpmap, sp = lineage_data(SIZES, 130, seed=21, missing=0.15, p_within=0.2, left_out=1)
    assert tmparr.shape == (17, 130) and (sp == -1).sum() == 1
    ssets = np.array([[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4], [0, 2, 3, 4], [1, 2, 3, 4]], np.uint32)
    return tmparr, sp, ssets


@pytest.mark.parametrize("shape", ["B1", "B5", "one_site_blocks"])
def test_model_routes_agree(case, shape):
    tmparr, sp, ssets = case
    starts = {"B1": [0, 130], "B5": [0, 7, 40, 41, 100, 130], "one_site_blocks": list(range(20, 61))}[shape]
    lit = sbm.literal_rows(tmparr, sp, len(SIZES), ssets, starts)
    fac = sbm.factored_rows_of(tmparr, sp, len(SIZES), ssets, starts)
    assert lit.shape == (5, len(starts) - 1, 16) and lit.dtype == np.uint32
    assert np.array_equal(lit, fac)
    assert lit[:, :, 15].any() and not lit[:, :, 0].any()
    assert np.array_equal(lit[:, :, 15].astype(np.int64), lit[:, :, 1:15].sum(axis=2, dtype=np.int64))


def random_counts(rng, n):
    """n count quadruples [n, 4, 4]: every species holds up to 255 lineages, spread over the bases, some missing"""
    size = rng.integers(0, 256, size=(n, 4))
    small = rng.random((n, 4)) < 0.3
    size[small] = rng.integers(0, 6, size=int(small.sum()))                 # small species beside large ones
    out = np.zeros((n, 4, 4), np.int64)
    for i in range(n):
        for k in range(4):
            present = int(rng.integers(0, size[i, k] + 1))                  # the rest is missing at this site
            p = rng.dirichlet(np.full(4, float(rng.choice([0.2, 1.0, 5.0]))))
            out[i, k] = rng.multinomial(present, p)
    return out


def test_site_rule_equals_enumeration_on_random_counts(lib):
    rng = np.random.default_rng(5)
    counts = random_counts(rng, 2000)
    assert counts.sum(axis=2).max() <= 255 and counts.sum(axis=2).max() > 200
    for c in counts:
        got, want = pooled(lib, c), sbm.site_row(c)
        assert np.array_equal(got.astype(np.int64), want), c
        assert got[0] == 0 and int(got[15]) == int(got[1:15].astype(np.int64).sum())


def test_site_rule_designed_counts(lib):
    z = np.zeros((4, 4), np.int64)
    assert not pooled(lib, z).any()                                          # all-zero counts
    one_missing = np.array([[3, 1, 0, 2], [0, 0, 0, 0], [5, 5, 1, 0], [2, 0, 0, 7]])
    assert not pooled(lib, one_missing).any() and not sbm.site_row(one_missing).any()
    # four species of 255 agreeing lineages: A, A, C, C -> class 0011 holds 255^4 (bit 31 set), and so does the sum
    agree = z.copy()
    agree[0, 0] = agree[1, 0] = agree[2, 1] = agree[3, 1] = 255
    got = pooled(lib, agree)
    want = np.zeros(16, np.int64)
    want[3] = want[15] = 255**4
    assert 255**4 == 4228250625 and 255**4 >= 2**31
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(sbm.site_row(agree), want)
    # every pair of classes: the 255s on two bases in every arrangement of the four species
    for p in range(1, 15):
        arr = z.copy()
        for k in range(4):
            arr[k, (p >> k) & 1] = 255
        assert np.array_equal(pooled(lib, arr).astype(np.int64), sbm.site_row(arr)), p
    # four species holding 255 on the same base: the pattern is invariant and counts nowhere
    same = z.copy()
    same[:, 2] = 255
    assert not pooled(lib, same).any() and not sbm.site_row(same).any()
    # 255 spread over all four bases in all four species
    spread = np.array([[64, 64, 64, 63], [63, 64, 64, 64], [1, 2, 3, 249], [100, 100, 55, 0]])
    assert np.array_equal(pooled(lib, spread).astype(np.int64), sbm.site_row(spread))


def test_unit_vectors_land_in_their_class(lib):
    """What the library's static_assert states, seen from outside: one lineage per species is one pattern."""
    cls = sbm.pattern_classes()
    for p in range(256):
        x = [(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3]
        c = np.zeros((4, 4), np.int64)
        c[np.arange(4), x] = 1
        want = np.zeros(16, np.int64)
        if cls[p]:
            want[cls[p]] = want[15] = 1
        assert np.array_equal(pooled(lib, c).astype(np.int64), want), p


def test_null_pointers_are_refused(lib):
    out = np.zeros(16, np.uint32)
    assert lib.tq_pooled_site_classes(None, out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert lib.tq_pooled_site_classes(out.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert b"tq_pooled_site_classes" in lib.tq_last_error(None)
