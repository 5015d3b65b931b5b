"""Pure Python / NumPy model of the five-taxon block rows, of the relabelling of A/B patterns and of the jackknife on sums
of slots.

Block rows come from the raw `tmparr` columns: missing is any code above 3, "two distinct values" is a literal count of
the values present in the column, the class is read off the four comparisons with row 0.  Nothing here knows about bit
planes or masks of sites.  The relabelling enumerates the two polarisations of a pattern on the ascending order and
takes the one whose position 0 is 'A'.  The jackknife is `blocks_model.jackknife_row` on Python ints.
"""
from __future__ import annotations

from itertools import product

import numpy as np

import blocks_model as bm


def column_classes(cols):
    """cols int[5, n] -> (i64[n] class 1..15 or 0 for a column that is not counted, bool[n] invariant and complete)."""
    cols = np.asarray(cols).astype(np.int64)
    complete = (cols <= 3).all(axis=0)
    ndistinct = sum(((cols == v).any(axis=0)).astype(np.int64) for v in range(4))
    k = sum((cols[i] != cols[0]).astype(np.int64) << (i - 1) for i in range(1, 5))
    counted = complete & (ndistinct == 2)
    return np.where(counted, k, 0), complete & (ndistinct == 1)


def block_rows(tmparr, sets5, block_starts) -> np.ndarray:
    """u32[Q,B,16]: per set and block slot k = the number of counted columns of class k, slot 0 their sum."""
    tmparr = np.asarray(tmparr)
    sets5 = np.asarray(sets5).reshape(-1, 5)
    starts = [int(v) for v in np.asarray(block_starts).reshape(-1)]
    B = len(starts) - 1
    out = np.zeros((sets5.shape[0], B, 16), np.uint32)
    for i, q in enumerate(sets5):
        k, _ = column_classes(tmparr[q.astype(np.int64)])
        for j in range(B):
            c = np.bincount(k[starts[j]:starts[j + 1]], minlength=16)
            out[i, j, 1:] = c[1:]
            out[i, j, 0] = c[1:].sum()
    return out


def invariant_sites(tmparr, set5, s0, s1) -> int:
    """Columns of [s0, s1) where the five taxa are all present and all equal."""
    _, inv = column_classes(np.asarray(tmparr)[np.asarray(set5, np.int64)][:, s0:s1])
    return int(inv.sum())


def class_table() -> np.ndarray:
    """u8[1024], index 256 x0 + 64 x1 + 16 x2 + 4 x3 + x4: 0 = not counted, else the class."""
    out = np.zeros(1024, np.uint8)
    for x in product(range(4), repeat=5):
        if len(set(x)) == 2:
            out[256 * x[0] + 64 * x[1] + 16 * x[2] + 4 * x[3] + x[4]] = sum(2 ** (i - 1) for i in range(1, 5) if x[i] != x[0])
    return out


def relabel(pattern: str, test) -> int:
    """The slot of `pattern` (letters in role order) for the taxa `test` (in role order): write the letters in ascending
    taxon order, take of that string and its A/B exchange the one that starts with 'A', read the class off it."""
    letter = {int(t): c for t, c in zip(test, pattern)}
    asc = "".join(letter[t] for t in sorted(letter))
    flipped = "".join("A" if c == "B" else "B" for c in asc)
    chosen = [s for s in (asc, flipped) if s[0] == "A"]
    assert len(chosen) == 1
    return sum(2 ** (i - 1) for i in range(1, 5) if chosen[0][i] == "B")


def masks(tests, stats) -> np.ndarray:
    """u16[N, len(stats), 2] slot masks of every test and statistic."""
    out = np.zeros((len(tests), len(stats), 2), np.uint16)
    for t, test in enumerate(tests):
        for s, sides in enumerate(stats):
            for side, pats in enumerate(sides):
                m = 0
                for pat in pats:
                    m |= 1 << relabel(pat, test)
                out[t, s, side] = m
    return out


def mask_sum(row, mask: int) -> int:
    return sum(int(row[k]) for k in range(16) if (int(mask) >> k) & 1)


def jackknife_masks_model(bclasses, set_of, lmask, rmask) -> np.ndarray:
    """f64[N,4] for block rows [M,B,16]: a_j, b_j = Python-int sums over the mask bits."""
    bclasses = np.asarray(bclasses)
    out = np.zeros((len(set_of), 4), np.float64)
    for t in range(len(set_of)):
        rows = bclasses[int(set_of[t])]
        out[t] = bm.jackknife_row([mask_sum(r, lmask[t]) for r in rows], [mask_sum(r, rmask[t]) for r in rows])
    return out


def jackknife_case(N: int, B: int, seed: int = 0):
    """Designed input of the mask jackknife: block rows u32[M,B,16], set_of u32[N], lmask / rmask u16[N] (valid: bit 0
    clear, non-empty, disjoint).  Test 0 reads 2^32 - 1 in every slot of every block, test 1 has left < right in every
    block, test 2 has every block empty, test 3 exactly one non-empty block (g = 1); the rest is random with empty
    blocks sprinkled in.  The special tests own their set."""
    rng = np.random.default_rng([seed, N, B, 5])
    M = max(4, (N + 1) // 2)
    set_of = rng.integers(0, M, size=N).astype(np.uint32)
    for t in range(min(N, 4)):
        set_of[t] = t
    if N > 4:
        set_of[4:] = rng.integers(4, M, size=N - 4) if M > 4 else 0
    lmask, rmask = np.zeros(N, np.uint16), np.zeros(N, np.uint16)
    for t in range(N):
        side = rng.integers(0, 3, size=15)                     # 0: unused, 1: left, 2: right
        side[rng.integers(0, 15)] = 1
        free = np.flatnonzero(side != 1)
        side[free[rng.integers(0, len(free))]] = 2
        lmask[t] = sum(1 << (k + 1) for k in range(15) if side[k] == 1)
        rmask[t] = sum(1 << (k + 1) for k in range(15) if side[k] == 2)
    rows = rng.integers(0, 3000, size=(M, B, 16)).astype(np.uint32)
    rows[rng.random((M, B, 16)) < 0.1] = 0
    rows[rng.random((M, B)) < 0.15] = 0                        # blocks with m_j = 0 for every test
    big = rng.random((M, B, 16)) < 0.02
    rows[big] = rng.integers(2**31, 2**32, size=int(big.sum()), dtype=np.uint64).astype(np.uint32)
    if N > 0:
        rows[0] = 0xFFFFFFFF
    if N > 1:
        for j in range(B):
            for k in range(1, 16):
                rows[1, j, k] = 3 + (j + k) % 7 if (int(lmask[1]) >> k) & 1 else 0xFFFFFF00 - j - k
    if N > 2:
        rows[2] = 0
    if N > 3:
        rows[3] = 0
        rows[3, B // 2, 1:] = np.arange(1, 16) * 3
    return rows, set_of, lmask, rmask
