"""An exact model of the rank space of quartets, in Python integers only: no numpy dtype takes part
in the arithmetic, so nothing here can wrap at 2^32, 2^53, 2^63 or 2^64.  Written from the definitions and the documented
construction of the sampler, with no library call.

    choose4(T)                  # C(T, 4)
    fits(T)                     # C(T, 4) < 2^64: T <= T_MAX = 145 056
    unrank_walk(rank, T)        # the lexicographic rule taxon by taxon (a loop over T): the definition
    unrank(rank, T)             # the same tuple by bisection on exact block starts (what the tests use at large T)
    unrank_many(ranks, T)       # u32 [Q, 4]
    half_bits(N)                # the smallest h >= 1 with 4^h >= N, capped at 32
    round_keys(seed)            # six 32-bit keys from a splitmix64 chain
    feistel(v, h, keys)         # six balanced rounds on 2h bits
    sampler(seed, N, Q)         # the first Q values of the cycle-walked permutation of [0, N)
    rank_list(T, seed)          # the ranks the unranking tests use at T
"""
from __future__ import annotations

import random
from math import comb

import numpy as np

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
T_MAX = 145_056                 # the last T whose C(T, 4) is below 2^64
ROUNDS = 6

#: tiny spaces (half_bits 1..4); C crosses 2^32 (half_bits 16 -> 17); the key regimes of the sort; sort on / off; the old
#: cap of tq_unrank (half_bits 31); the first T at which T(T-1)/2 (T-2)/3 (T-3) wraps and the first half_bits 32; the last
T_LIST = (4, 5, 7, 8, 568, 569, 1625, 1626, 65_535, 65_536, 100_000, 102_570, 102_571, T_MAX)


def choose4(T: int) -> int:
    return comb(T, 4)


def fits(T: int) -> bool:
    return choose4(T) < 1 << 64


def unrank_walk(rank: int, T: int) -> tuple:
    """Taxon t joins the combination when the combinations that hold it (with what is picked so far) reach past the
    rank; otherwise they are skipped."""
    assert 0 <= rank < choose4(T)
    picked = []
    for t in range(T):
        need = 4 - len(picked)
        if need == 0:
            break
        block = comb(T - t - 1, need - 1)       # combinations whose next taxon is t
        if rank < block:
            picked.append(t)
        else:
            rank -= block
    return tuple(picked)


def unrank(rank: int, T: int) -> tuple:
    """With k picks left among the taxa p..T-1, the combinations whose next taxon is below t number
    C(T-p, k) - C(T-t, k), which grows with t: the pick is the largest t at which that is <= the rank left."""
    assert 0 <= rank < choose4(T)
    picked, p = [], 0
    for k in (4, 3, 2, 1):
        whole = comb(T - p, k)
        lo, hi = p, T - k
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if whole - comb(T - mid, k) <= rank:
                lo = mid
            else:
                hi = mid - 1
        rank -= whole - comb(T - lo, k)
        picked.append(lo)
        p = lo + 1
    assert rank == 0
    return tuple(picked)


def unrank_many(ranks, T: int) -> np.ndarray:
    return np.array([unrank(int(r), T) for r in ranks], np.uint32).reshape(-1, 4)


def half_bits(N: int) -> int:
    h = 1
    while h < 32 and 4 ** h < N:
        h += 1
    return h


def round_keys(seed: int) -> list:
    """splitmix64 (Steele, Lea & Flood 2014): the state steps by the golden-ratio constant, each output is the finalised
    state; a round key is bits 16..47 of an output."""
    keys, x = [], seed & M64
    for _ in range(ROUNDS):
        x = (x + 0x9E3779B97F4A7C15) & M64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        keys.append((z >> 16) & M32)
    return keys


def lowbias32(x: int) -> int:
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def feistel(v: int, h: int, keys) -> int:
    mask = (1 << h) - 1
    left, right = (v >> h) & mask, v & mask
    for key in keys:
        left, right = right, left ^ (lowbias32(right ^ key) & mask)
    return (left << h) | right


def sampler(seed: int, N: int, Q: int) -> list:
    """Element i of the sample is i sent through the permutation of [0, 4^h) until it lands below N."""
    assert 0 <= Q <= N
    h, keys = half_bits(N), round_keys(seed)
    out = []
    for i in range(Q):
        v = feistel(i, h, keys)
        while v >= N:
            v = feistel(v, h, keys)
        out.append(v)
    return out


def rank_list(T: int, seed: int = 0) -> list:
    """Both ends, the 32-, 53- and 63-bit boundaries, the ranks at which the first taxon changes, and 200 seeded draws;
    each once, below C(T, 4), in a fixed order."""
    total = choose4(T)
    want = [0, 1, total - 1, total - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**53 - 1, 2**53 + 1, 2**63 - 1, 2**63, 2**63 + 1]
    for a in (1, 2, T // 2, T - 4):
        first = total - choose4(T - a)          # the first rank whose combination starts with taxon a
        want += [first, first - 1]
    rng = random.Random(1000 * T + seed)
    want += [rng.randrange(total) for _ in range(200)]
    return list(dict.fromkeys(r for r in want if 0 <= r < total))
