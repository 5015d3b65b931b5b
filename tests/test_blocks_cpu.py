"""CPU: the block jackknife's host execution against Python floats bit for bit, an independent variance formula, the
refusals, `locus_blocks` and `jackknife_moments`."""
import ctypes
import math

import numpy as np
import pytest

import blocks_model as bm


@pytest.fixture(scope="module")
def patterns():
    from tetrad_amd import _lib, patterns
    _lib.build()
    return patterns


@pytest.mark.parametrize("B", [1, 2, 3, 50, 4096])
@pytest.mark.parametrize("N", [1, 64, 65, 1000])
def test_host_equals_python_floats(patterns, N, B):
    rows, set_of, ia, ib = bm.jackknife_case(N, B)
    got = patterns.dstat_jackknife(rows, set_of, ia, ib)
    want = bm.jackknife_model(rows, set_of, ia, ib)
    assert got.shape == (N, 4)
    assert np.array_equal(bm.bits(got), bm.bits(want))
    # the designed tests are what their names say
    assert got[0, 0] == B and got[0, 1] == 0.0                          # counts of 2^32 - 1: a = b
    if N > 1:
        assert got[1, 1] < 0                                            # a < b everywhere
    if N > 2:
        assert got[2, 0] == 0 and np.isnan(got[2, 1:]).all()            # every block empty
    if N > 3:
        assert got[3, 0] == 1 and got[3, 1] == 7 / 15 and np.isnan(got[3, 2:]).all()     # g = 1
    if N > 4 and B > 1:
        assert got[4, 0] == 2 and np.isfinite(got[4]).all()             # two non-empty blocks


def test_nan_is_the_quiet_nan_of_python(patterns):
    rows = np.zeros((1, 3, 16), np.uint32)
    out = patterns.dstat_jackknife(rows, [0], [8], [6])
    assert [int(v) for v in bm.bits(out)[0, 1:]] == [bm.NAN_BITS] * 3
    assert int(bm.bits(np.array([math.nan]))[0]) == bm.NAN_BITS


@pytest.mark.parametrize("g", [2, 3, 7, 50, 400])
def test_equal_weights_give_the_plain_jackknife_variance(patterns, g):
    """With the same m_j in every block h = g for all j, and the weighted variance is the plain delete-one variance
    (g - 1) / g * sum (theta_-j - mean theta_-j)^2.  Both sides are f64 evaluations of one real number: relative
    1e-9 is loose against their rounding (about g 2^-53) and far below any error in the formula."""
    rng = np.random.default_rng(g)
    m = 1000
    a = rng.integers(0, m + 1, size=g)
    rows = np.zeros((1, g + 2, 16), np.uint32)
    used = np.r_[0, np.arange(2, g + 1)]                                # blocks 1 and g + 1 stay empty
    rows[0, used, 8] = a
    rows[0, used, 6] = m - a
    out = patterns.dstat_jackknife(rows, [0], [8], [6])[0]
    d = 2.0 * a - m                                                     # a_j - b_j
    loo = (d.sum() - d) / float((g - 1) * m)
    plain = (g - 1) / g * ((loo - loo.mean()) ** 2).sum()
    assert out[0] == g
    assert plain > 0
    assert abs(out[3] - plain) <= 1e-9 * plain
    # and theta_J = g theta - (g - 1) mean theta_-j
    tj = g * (d.sum() / float(g * m)) - (g - 1) * loo.mean()
    assert abs(out[2] - tj) <= 1e-9 * max(abs(tj), 1.0)


def test_refusals_leave_out_untouched(patterns):
    from tetrad_amd import _lib
    lib = _lib.load()
    rows, set_of, ia, ib = bm.jackknife_case(8, 3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(rows_, n_sets, B, set_of_, ia_, ib_, N):
        out = np.full((8, 4), -7.0)
        rc = lib.tq_dstat_jackknife(p(rows_), n_sets, B, p(set_of_), p(ia_), p(ib_), N, p(out))
        return rc, out

    rc, out = call(rows, rows.shape[0], 3, set_of, ia, ib, 8)
    assert rc == 0 and not (out == -7.0).any()
    bad_set = set_of.copy()
    bad_set[5] = rows.shape[0]
    bad_ia = ia.copy()
    bad_ia[7] = 15
    bad_ib = ib.copy()
    bad_ib[0] = 200
    # the full texts, as the library gave them before the checks of the two test forms became one
    for args, text in [((rows, rows.shape[0], 3, bad_set, ia, ib, 8), b"test 5 has set_of=5 >= n_sets=5"),
                       ((rows, rows.shape[0], 3, set_of, bad_ia, ib, 8), b"test 7 has a class index above 14 (15, 8)"),
                       ((rows, rows.shape[0], 3, set_of, ia, bad_ib, 8), b"test 0 has a class index above 14 (8, 200)"),
                       ((rows, rows.shape[0], 0, set_of, ia, ib, 8), b"B=0 blocks, must be 1..4096"),
                       ((rows, rows.shape[0], 4097, set_of, ia, ib, 8), b"B=4097 blocks, must be 1..4096"),
                       ((rows, -1, 3, set_of, ia, ib, 8), b"NULL pointer or negative size"),
                       ((rows, rows.shape[0], 3, set_of, ia, ib, -1), b"NULL pointer or negative size")]:
        rc, out = call(*args)
        assert rc == -1 and (out == -7.0).all(), text
        assert lib.tq_last_error(None) == b"tq_dstat_jackknife: " + text
    out = np.full((8, 4), -7.0)
    assert lib.tq_dstat_jackknife(None, 5, 3, p(set_of), p(ia), p(ib), 8, p(out)) == -1 and (out == -7.0).all()
    assert lib.tq_dstat_jackknife(p(rows), 5, 3, p(set_of), p(ia), p(ib), 8, None) == -1
    assert lib.tq_dstat_jackknife(None, 0, 3, None, None, None, 0, None) == 0           # N = 0 is valid
    with pytest.raises(ValueError):
        patterns.dstat_jackknife(rows[:, :, :15], set_of, ia, ib)
    with pytest.raises(ValueError):
        patterns.dstat_jackknife(rows, set_of, ia[:3], ib)


def locus_column(widths):
    return np.repeat(np.arange(len(widths), dtype=np.uint32) * 3 + 5, widths)


@pytest.mark.parametrize("nblocks", [1, 2, 7, 50, 4096])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_locus_blocks(patterns, nblocks, seed):
    rng = np.random.default_rng(seed)
    widths = rng.integers(1, 40, size=[3, 60, 500][seed])
    locus = locus_column(widths)
    S = int(widths.sum())
    for tmpmap in (locus, np.stack([locus, np.arange(S, dtype=np.uint32)], axis=1)):
        starts = patterns.locus_blocks(tmpmap, nblocks)
        assert starts.dtype == np.int64
        B = min(nblocks, len(widths))
        assert starts.shape == (B + 1,)
        assert starts[0] == 0 and starts[-1] == S and (np.diff(starts) > 0).all()
        edges = set(np.concatenate([[0], np.cumsum(widths)]).tolist())
        assert set(starts.tolist()) <= edges
        assert np.array_equal(starts, patterns.locus_blocks(tmpmap, nblocks))          # deterministic
    if B == len(widths):
        assert np.array_equal(starts, np.concatenate([[0], np.cumsum(widths)]))
    elif len(widths) >= 10 * B:
        # many small loci per block: no cut is further than one locus from its equal-sites target
        target = np.arange(B + 1) * S / B
        assert np.abs(starts - target).max() <= widths.max()


def test_locus_blocks_small_cases(patterns):
    assert patterns.locus_blocks(np.zeros(17, np.uint32), 50).tolist() == [0, 17]        # one locus
    assert patterns.locus_blocks(np.zeros(1, np.uint32), 1).tolist() == [0, 1]
    # equal loci: the equal-sites cuts exactly
    assert patterns.locus_blocks(locus_column([10] * 12), 4).tolist() == [0, 30, 60, 90, 120]
    # one huge locus in front: the later cuts still find a boundary each
    assert patterns.locus_blocks(locus_column([100, 1, 1, 1]), 4).tolist() == [0, 100, 101, 102, 103]
    assert patterns.locus_blocks(locus_column([1, 1, 1, 100]), 4).tolist() == [0, 1, 2, 3, 103]
    # a tie between two boundaries goes to the lower one
    assert patterns.locus_blocks(locus_column([4, 2, 4]), 2).tolist() == [0, 4, 10]
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            patterns.locus_blocks(np.zeros(5, np.uint32), bad)
    with pytest.raises(ValueError):
        patterns.locus_blocks(np.zeros(0, np.uint32), 3)


def test_jackknife_moments(patterns):
    out = np.array([[0.0, math.nan, math.nan, math.nan], [1.0, 0.25, math.nan, math.nan], [5.0, -0.5, -0.49, 0.0004],
                    [2.0, 0.1, 0.1, 0.0]])
    g, mean, se = patterns.jackknife_moments(out)
    assert g.dtype == np.int64 and g.tolist() == [0, 1, 5, 2]
    assert np.isnan(mean[:2]).all() and mean[2:].tolist() == [-0.49, 0.1]
    assert np.isnan(se[:2]).all() and se[2] == math.sqrt(0.0004) and se[3] == 0.0
