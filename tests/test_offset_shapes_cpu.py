"""CPU: the shapes of tests/offset_shapes.py lie where tests/test_gpu_offset_range.py needs them -- on both sides of
bit 31 of a 32-bit row offset, of the host's limit for the cooperative scan kernels and of 2^32 -- and their inputs can
tell a mis-addressed row from the right one."""
from itertools import combinations

import numpy as np
import pytest

import offset_shapes as osh

# written out here, not imported from the code under test
TWO31 = 2147483648
LIMIT = 0xFFFF0000            # the host keeps a batch on the cooperative kernels only while T * pitch < LIMIT
TWO32 = 4294967296
PB_MAX_TILES = 1023           # steps the 16-bit counters of the bank-private form allow (scan_pb.hpp)


def test_shape_table():
    assert osh.S == 1_400_000 and osh.SP == 1_400_832 and osh.SP % 2048 == 0 and osh.SP - osh.S < 2048
    assert osh.SP // 2048 == 684 <= PB_MAX_TILES
    assert osh.T_ROWS == 3067 == max(osh.SHAPES)
    assert [T * osh.SP for T in osh.SHAPES] == [2_241_331_200, 4_293_550_080, 4_294_950_912, 4_296_351_744]
    a, b, c, d = (T * osh.SP for T in osh.SHAPES)
    assert TWO31 < a < LIMIT and 1600 ** 3 <= TWO32           # bit 31 set; keys of the joint-histogram scan hold (a,b,c)
    assert 1625 ** 3 <= TWO32 < 1626 ** 3 and TWO31 / 1625 > 1.32e6   # dp needs T <= 1625: bit 31 needs S >= 1.33e6
    assert LIMIT - b == 1_351_680 and 3065 ** 3 > TWO32       # just inside; dp not eligible
    assert LIMIT <= c < TWO32                                 # the band only the host comparison guards
    assert d >= TWO32
    # row 1533 starts 8 192 bytes below 2^31 and straddles it; rows 1532 / 1534 lie on either side
    assert TWO31 - 1533 * osh.SP == 8192 and 1534 * osh.SP > TWO31 > 1533 * osh.SP
    # every shape's last rows end within the last row of its range
    for T in osh.SHAPES:
        rows = osh.hot_rows(T)
        assert len(rows) == 9 == len(set(rows)) and max(rows) == T - 1 and set(rows) <= set(osh.ALL_HOT)
    assert len(osh.ALL_HOT) == 15


def test_packed_pitch_is_inside_at_1600_and_past_the_limit_at_3065():
    """Six 5-site loci per 32-site word: the packed pitch is about 1.07 times the natural one."""
    from tetrad_amd.engine import PACK_PAD, pack_sites
    _, _, tmpmap = osh.simulated()
    src = pack_sites(tmpmap)
    psp = len(src)
    assert psp % 2048 == 0 and 1.06 * osh.SP < psp < 1.08 * osh.SP
    assert np.array_equal(np.sort(src[src != PACK_PAD]), np.arange(osh.S))
    assert TWO31 < 1600 * psp < LIMIT
    assert 3065 * psp >= LIMIT > 3065 * osh.SP


def test_quartets_cover_shared_and_own_positions():
    for T in osh.SHAPES:
        q, idx = osh.quartets(T)
        assert q.shape == (252, 4) and q.dtype == np.uint32 and len(q) >= 2 * 64
        lex = np.array(list(combinations(osh.hot_rows(T), 4)), np.uint32)
        assert np.array_equal(q[:126], lex) and np.array_equal(q, lex[idx])
        assert sorted(idx[126:].tolist()) == list(range(126)) and not np.array_equal(idx[126:], np.arange(126))
        assert (np.diff(q.astype(np.int64), axis=1) > 0).all() and q.max() == T - 1
        # the straddling row and the last rows occur in the shared positions (a, b) and in the own ones (c, d)
        for r in (1533, T - 4, T - 3):
            assert (q[:, :2] == r).any() and (q[:, 2:] == r).any()
        assert (q[:, 2:] == T - 1).any() and (q[:, 1] == T - 3).any()


def test_hot_rows_differ_from_each_other_and_from_the_decoy():
    hot, decoy, tmpmap = osh.simulated()
    assert hot.shape == (15, osh.S) and decoy.shape == (osh.S,) and tmpmap.shape == (osh.S, 2)
    assert np.array_equal(tmpmap[:, 0], np.arange(osh.S) // 5)
    assert set(np.unique(hot).tolist()) == {0, 1, 2, 3, 78}
    rows = list(hot) + [decoy]
    for i, j in combinations(range(len(rows)), 2):
        share = float((rows[i] != rows[j]).mean())
        assert share > 0.5, (i, j, share)


@pytest.mark.parametrize("T", osh.SHAPES)
def test_oracle_counts_something_for_every_quartet(oracle, T):
    for sub in (False, True):
        rstat, rscor, dbg, exact = osh.expected(T, sub)
        assert rstat.shape == (252, 2) and (rstat[:, 1] > 0).all()
        assert np.array_equal(rstat[:126][osh.quartets(T)[1][126:]], rstat[126:])
        # subsample mode counts at most one site per locus, full mode every variable site without a missing base
        n_loci = osh.S // 5
        assert (rstat[:, 1] <= (n_loci if sub else osh.S)).all()
    full, subs = osh.expected(T, False)[0], osh.expected(T, True)[0]
    assert (subs[:, 1] < full[:, 1]).all()
