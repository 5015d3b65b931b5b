"""The exact model of the rank space (tests/rank_model.py) against what pins it -- itertools, the reference's own
unranking in tests/golden/host_f2f3.npz, the permutation property of the sampler's construction -- and the library's host
unranker `tq_unrank` against the model over the whole 64-bit rank space: every T of rank_model.T_LIST, ranks up to
C(145 056, 4) - 1 = 2^64 - 1.6e14, and the refusals at the ends of the space.  No GPU."""
from itertools import combinations

import numpy as np
import pytest

import rank_model as rm
from conftest import load_golden
from tetrad_amd import combinations as C
from tetrad_amd._lib import TetradHipError

INVALID_ARG = "TQ_ERR_INVALID_ARG"
SEEDS = (0, 1, 2**63, 2**64 - 1)


def test_the_limits_of_the_space():
    """The figures the library's comments and messages quote."""
    assert rm.choose4(rm.T_MAX) < 2**64 <= rm.choose4(rm.T_MAX + 1) and rm.fits(rm.T_MAX) and not rm.fits(rm.T_MAX + 1)
    assert rm.choose4(102_571) == 4_611_707_052_270_601_010
    wraps = lambda T: T * (T - 1) // 2 * (T - 2) // 3 * (T - 3) >= 2**64        # noqa: E731
    assert wraps(102_571) and not wraps(102_570)
    assert rm.choose4(102_570) < 2**62 < rm.choose4(102_571)
    assert rm.choose4(568) < 2**32 < rm.choose4(569)
    assert [rm.half_bits(rm.choose4(T)) for T in rm.T_LIST] == [1, 2, 3, 4, 16, 17, 20, 20, 30, 30, 31, 31, 32, 32]
    assert 1625**3 <= 0xFFFFFFFF < 1626**3 and 65_535**2 <= 0xFFFFFFFF < 65_536**2


@pytest.mark.parametrize("T", range(4, 13))
def test_model_unranks_in_itertools_order(T):
    want = list(combinations(range(T), 4))
    assert len(want) == rm.choose4(T)
    assert [rm.unrank_walk(r, T) for r in range(len(want))] == want
    assert [rm.unrank(r, T) for r in range(len(want))] == want


@pytest.mark.parametrize("T", [16, 64, 128, 256])
def test_model_equals_the_reference_fixture(T):
    g = load_golden("host_f2f3")
    ranks, want = g[f"unrank_T{T}_ranks"], g[f"unrank_T{T}_quartets"]
    np.testing.assert_array_equal(rm.unrank_many(ranks, T), want)
    assert [rm.unrank_walk(int(r), T) for r in ranks] == [tuple(q) for q in want.tolist()]


@pytest.mark.parametrize("T", [569, 102_571, rm.T_MAX])
def test_bisection_equals_the_walk_at_large_t(T):
    """The walk over all taxa is the definition; the bisection is what the tests can afford at 4 096 ranks per case."""
    total = rm.choose4(T)
    ranks = [0, total - 1, total - rm.choose4(T // 2), 2**32, 2**63 + 1] + rm.rank_list(T)[-8:]
    for r in (r for r in ranks if r < total):
        assert rm.unrank(r, T) == rm.unrank_walk(r, T)


@pytest.mark.parametrize("h", range(1, 7))
def test_feistel_is_a_bijection(h):
    for seed in SEEDS:
        keys = rm.round_keys(seed)
        assert len(keys) == 6 and all(0 <= k < 2**32 for k in keys)
        image = sorted(rm.feistel(v, h, keys) for v in range(4**h))
        assert image == list(range(4**h))


def test_round_keys_are_a_splitmix64_chain():
    """The first outputs of splitmix64 from state 0 are published test vectors (Vigna's splitmix64.c)."""
    out = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC, 0x1B39896A51A8749B, 0x53CB9F0C747EA2EA]
    assert rm.round_keys(0) == [(z >> 16) & 0xFFFFFFFF for z in out]
    assert rm.round_keys(2**64 - 1)[1:] == rm.round_keys(0x9E3779B97F4A7C15 - 1)[:5]    # one step further down the chain


@pytest.mark.parametrize("T", range(4, 28))
def test_cycle_walk_is_a_permutation(T):
    """T = 4 | 5 | 7 | 8 | 11 | 15 | 20 | 27 are the first T of half_bits 1..8."""
    N = rm.choose4(T)
    for seed in SEEDS:
        full = rm.sampler(seed, N, N)
        assert sorted(full) == list(range(N))
        assert rm.sampler(seed, N, N // 3) == full[:N // 3]


def test_half_bits_steps():
    firsts = {}
    for T in range(4, 28):
        firsts.setdefault(rm.half_bits(rm.choose4(T)), T)
    assert firsts == {1: 4, 2: 5, 3: 7, 4: 8, 5: 11, 6: 15, 7: 20, 8: 27}
    assert [rm.half_bits(N) for N in (1, 4, 5, 16, 17, 2**62, 2**62 + 1, 2**64 - 1)] == [1, 1, 2, 2, 3, 31, 32, 32]


@pytest.mark.parametrize("T", rm.T_LIST)
def test_host_unrank_equals_the_model(T):
    """tq_unrank over the rank list: as an array of ranks, and as ranges of one and two ranks around each of them."""
    ranks = rm.rank_list(T)
    want = rm.unrank_many(ranks, T)
    np.testing.assert_array_equal(C.unrank(np.array(ranks, np.uint64), T), want)
    total = rm.choose4(T)
    for r, w in list(zip(ranks, want))[:24]:
        np.testing.assert_array_equal(C.unrank(None, T, r, 1), w[None])
        if r + 1 < total:
            np.testing.assert_array_equal(C.unrank(None, T, r, 2), [w, rm.unrank(r + 1, T)])


@pytest.mark.parametrize("T", [8, 569, 102_571, rm.T_MAX])
def test_host_unrank_refuses_ranges_past_the_space(T):
    total = rm.choose4(T)
    with pytest.raises(TetradHipError, match=INVALID_ARG + r".*rank range \[18446744073709551615,\+2\) exceeds C\(%d,4\)" % T):
        C.unrank(None, T, 2**64 - 1, 2)             # the sum first_rank + Q wraps to 1
    for first, count in ((total, 1), (total - 1, 2), (total + 1, 1)):
        with pytest.raises(TetradHipError, match=INVALID_ARG):
            C.unrank(None, T, first, count)
    with pytest.raises(TetradHipError, match=INVALID_ARG):
        C.unrank([0, total], T)
    np.testing.assert_array_equal(C.unrank(None, T, total - 1, 1), [[T - 4, T - 3, T - 2, T - 1]])
    np.testing.assert_array_equal(C.unrank([total - 1], T), [[T - 4, T - 3, T - 2, T - 1]])


def test_host_unrank_refuses_a_rank_space_past_64_bits():
    for T in (rm.T_MAX + 1, 200_000, 2**31 - 1):
        with pytest.raises(TetradHipError, match=INVALID_ARG + r".*C\(%d,4\) does not fit 64 bits" % T):
            C.unrank([0], T)
        with pytest.raises(TetradHipError, match=INVALID_ARG + r".*C\(%d,4\) does not fit 64 bits" % T):
            C.unrank(None, T, 0, 1)
    np.testing.assert_array_equal(C.unrank([0], rm.T_MAX), [[0, 1, 2, 3]])          # the next valid call
