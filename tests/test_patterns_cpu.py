"""CPU-only: the class rule, the role permutation, the D test bookkeeping and the host execution of the accumulation."""
import ctypes
import math
from itertools import combinations, permutations, product

import numpy as np
import pytest

from conftest import load_golden
import patterns_model as pm
from tetrad_amd import _lib, patterns
from tetrad_amd._lib import TetradHipError


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def table(lib):
    return patterns.class_table()


def rule_class(x):
    seen = {}
    return pm.STRINGS.index("".join(str(seen.setdefault(b, len(seen))) for b in x))


def test_table_is_the_rule(table):
    assert patterns.CLASS_STRINGS == tuple(pm.STRINGS)
    for x in product(range(4), repeat=4):
        assert table[64 * x[0] + 16 * x[1] + 4 * x[2] + x[3]] == rule_class(x), x
    assert np.bincount(table, minlength=15).tolist() == pm.SIZES
    assert (table[[0b00000101, 0b00010001, 0b00010100]] == [patterns.BBAA, patterns.BABA, patterns.ABBA]).all()


def test_table_null_pointer(lib):
    assert lib.tq_pattern_class_table(None) == -1


def test_model_agrees_with_the_rule():
    pats = np.array(list(product(range(4), repeat=4)), np.uint8).T
    assert pm.site_classes(pats).tolist() == [rule_class(x) for x in pats.T.tolist()]


def test_permute_classes_is_a_recount(table):
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 1000, size=(6, 256))
    pats = np.array(list(product(range(4), repeat=4)))
    idx = lambda p: 64 * p[:, 0] + 16 * p[:, 1] + 4 * p[:, 2] + p[:, 3]
    classes = pm.table_classes(counts, table)
    for perm in permutations(range(4)):
        moved = np.zeros_like(counts)
        moved[:, idx(pats[:, list(perm)])] = counts[:, idx(pats)]       # the site with pattern x now shows x[perm]
        assert np.array_equal(patterns.permute_classes(classes, perm), pm.table_classes(moved, table)), perm
    assert np.array_equal(patterns.permute_classes(classes[:, :15], (1, 0, 3, 2))[:, 8], classes[:, 8])
    with pytest.raises(ValueError):
        patterns.permute_classes(classes, (0, 1, 2, 2))


@pytest.mark.parametrize("name", ["tiny_T5_S37", "edge_T7_S130"])
def test_dstat_tests_against_direct_counts(name):
    g = load_golden(name)
    tmparr, T = g["tmparr"], g["tmparr"].shape[0]
    tests = np.array([p for s in combinations(range(T), 4) for p in permutations(s)])
    tests = tests[np.random.default_rng(1).permutation(len(tests))]
    sets, set_of, ia, ib = patterns.dstat_tests(tests)
    assert sets.dtype == np.uint32 and set_of.dtype == np.uint32 and ia.dtype == np.uint8 and ib.dtype == np.uint8
    assert sets.shape == (math.comb(T, 4), 4) and (np.diff(sets.astype(np.int64), axis=1) > 0).all()
    assert len(np.unique(sets, axis=0)) == len(sets)
    assert np.array_equal(sets[set_of], np.sort(tests, axis=1))
    # invariant sites are class 0, which no test reads: counting them changes nothing here
    classes = pm.model_classes(tmparr, g["tmpmap"], sets, subsample=False)
    for t, test in enumerate(tests):
        assert (classes[set_of[t], ia[t]], classes[set_of[t], ib[t]]) == pm.direct_abba_baba(tmparr, test), test


def test_dstat_tests_refuses_bad_input():
    with pytest.raises(ValueError):
        patterns.dstat_tests([[0, 1, 1, 2]])
    with pytest.raises(ValueError):
        patterns.dstat_tests([[0, 1, 2]])
    with pytest.raises(ValueError):
        patterns.dstat_tests([[0, 1, 2, -3]])
    sets, set_of, ia, ib = patterns.dstat_tests(np.zeros((0, 4), np.int64))
    assert sets.shape == (0, 4) and len(set_of) == len(ia) == len(ib) == 0


def test_tests_with_outgroup():
    t = patterns.tests_with_outgroup(7, 2)
    assert t.shape == (3 * math.comb(6, 3), 4) and (t[:, 3] == 2).all()
    assert len({tuple(r) for r in t.tolist()}) == len(t)
    sets, set_of, ia, ib = patterns.dstat_tests(t)
    assert len(sets) == math.comb(6, 3) and np.bincount(set_of).tolist() == [3] * len(sets)
    # the three tests of a set put each of the three pairings in the ABBA / BABA places once
    for s in range(len(sets)):
        pairs = {frozenset((int(a), int(b))) for a, b in zip(ia[set_of == s], ib[set_of == s])}
        assert len(pairs) == 3 and set().union(*pairs) == {patterns.BBAA, patterns.BABA, patterns.ABBA}
    with pytest.raises(ValueError):
        patterns.tests_with_outgroup(5, 5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("N", [1, 64, 65, 1000])
def test_dstat_accumulate_matches_python_floats(lib, N):
    reps, set_of, ia, ib = pm.dstat_case(N)
    acc = np.zeros((N, 4), np.float64)
    for c in reps:
        patterns.dstat_accumulate(c, set_of, ia, ib, acc)
    model = np.array(pm.dstat_model(reps, set_of, ia, ib))
    assert np.array_equal(bits(acc), bits(model))
    assert acc[0, 0] == len(reps) and reps[0][set_of[0], ia[0]] == 2**32 - 1
    if N >= 4:
        assert (acc[1, 3] < 0) and acc[1, 0] == len(reps)
        assert not acc[2].any()                                          # a + b = 0 in every replicate: untouched
        assert 0 < acc[3, 0] < len(reps)                                 # ... and in some


def test_dstat_accumulate_refusals(lib):
    reps, set_of, ia, ib = pm.dstat_case(65)
    acc = np.full((65, 4), 7.5)
    for field, value in (("set_of", len(reps[0])), ("ia", 15), ("ib", 255)):
        bad = dict(set_of=set_of.copy(), ia=ia.copy(), ib=ib.copy())
        bad[field][40] = value
        with pytest.raises(TetradHipError) as e:
            patterns.dstat_accumulate(reps[0], bad["set_of"], bad["ia"], bad["ib"], acc)
        assert e.value.code == -1 and "test 40" in str(e.value)
        assert (acc == 7.5).all()
    assert lib.tq_dstat_accumulate(None, 1, None, None, None, 1, None) == -1
    assert lib.tq_dstat_accumulate(None, 0, None, None, None, 0, None) == 0
    assert lib.tq_dstat_accumulate_dev(None, None, 0, None, None, None, 0, None, None) == -1
    assert lib.tq_patterns(None, None, 0, 0, None) == -1 and lib.tq_patterns_species_dev(None, None, 0, None, None) == -1


def test_moments_and_nan_cases():
    D = np.array([0.25, 0.5, np.nan, 0.1, -0.3])
    acc = np.array([[4.0, 1.0, 0.5, 0.1],           # ordinary
                    [0.0, 0.0, 0.0, 0.0],           # no replicate counted
                    [3.0, 0.3, 0.2, 0.1],           # no observed D
                    [1.0, 0.2, 0.2 * 0.2, 0.2],     # one replicate: std = 0
                    [2.0, 0.2, 0.01, 0.1]])         # s2 / n - mean^2 slightly negative or zero: clamped
    n, mean, std, Z = patterns.dstat_moments(D, acc)
    assert n.tolist() == [4, 0, 3, 1, 2]
    m = 1.0 / 4.0
    s = math.sqrt(0.5 / 4.0 - m * m)
    assert mean[0] == m and std[0] == s and Z[0] == 0.25 / s
    assert np.isnan([mean[1], std[1], Z[1]]).all()
    assert np.isnan(Z[2]) and not np.isnan(std[2])
    assert std[3] == 0.0 and np.isnan(Z[3])
    assert std[4] == 0.0 and np.isnan(Z[4])
    want = pm.moments_model(D, acc.tolist())
    got = list(zip(n.tolist(), mean.tolist(), std.tolist(), Z.tolist()))
    assert np.array_equal(bits(np.array(got, float)), bits(np.array(want, float)))


def test_observed_columns():
    classes = np.zeros((2, 16), np.uint32)
    classes[0, [3, 6, 8, 15]] = [50, 10, 30, 100]
    out = patterns.observed_dstat(classes, [0, 1, 0], [8, 8, 6], [6, 6, 8], [3, 3, 3])
    assert out["abba"].tolist() == [30, 0, 10] and out["baba"].tolist() == [10, 0, 30] and out["bbaa"].tolist() == [50, 0, 50]
    assert out["nsites"].tolist() == [100, 0, 100]
    assert out["D"][0] == 20 / 40 and np.isnan(out["D"][1]) and out["D"][2] == -20 / 40
    assert (out["boot_n"] == 0).all() and np.isnan(out["Z"]).all()
