"""Pure Python / NumPy model of the per-block class rows and of the block jackknife.

Block rows come from the raw `tmparr` columns of the block through `patterns_model.site_classes` / `counted_sites`;
nothing here knows about bit planes.  `jackknife_model` is the six steps of the rule on Python ints and floats, one
operation per statement, in the order the rule gives them.
"""
from __future__ import annotations

import math

import numpy as np

import patterns_model as pm

NAN_BITS = 0x7FF8000000000000


def block_rows(tmparr, sets, block_starts, count_invariant: bool = False) -> np.ndarray:
    """u32[Q,B,16]: per set and block the 15 class counts of the block's columns and their sum (full mode)."""
    tmparr = np.asarray(tmparr)
    sets = np.asarray(sets).reshape(-1, 4)
    starts = [int(v) for v in np.asarray(block_starts).reshape(-1)]
    B = len(starts) - 1
    out = np.zeros((sets.shape[0], B, 16), np.uint32)
    for i, q in enumerate(sets):
        rows = tmparr[q.astype(np.int64)]
        for j in range(B):
            sl = rows[:, starts[j]:starts[j + 1]]
            idx = pm.counted_sites(sl, None, False, count_invariant)
            c = np.bincount(pm.site_classes(sl[:, idx]), minlength=15)
            out[i, j, :15] = c
            out[i, j, 15] = c.sum()
    return out


def jackknife_row(a, b):
    """One test: a, b = lists of the per-block ABBA and BABA counts (Python ints) -> [g, theta, theta_J, var]."""
    A = sum(a)
    Bs = sum(b)
    n = A + Bs
    g = sum(1 for x, y in zip(a, b) if x + y > 0)
    if n == 0:
        return [0.0, math.nan, math.nan, math.nan]
    nf = float(n)
    theta = float(A - Bs) / nf
    if g < 2:
        return [float(g), theta, math.nan, math.nan]
    sJ = 0.0
    for aj, bj in zip(a, b):
        m = aj + bj
        if m == 0:
            continue
        r = float(n - m)
        tj = float((A - aj) - (Bs - bj)) / r
        w = r / nf
        p = w * tj
        sJ = sJ + p
    gt = float(g) * theta
    theta_j = gt - sJ
    sV = 0.0
    for aj, bj in zip(a, b):
        m = aj + bj
        if m == 0:
            continue
        r = float(n - m)
        tj = float((A - aj) - (Bs - bj)) / r
        h = nf / float(m)
        h1 = h - 1.0
        ht = h * theta
        hj = h1 * tj
        tau = ht - hj
        e = tau - theta_j
        ee = e * e
        q = ee / h1
        sV = sV + q
    return [float(g), theta, theta_j, sV / float(g)]


def jackknife_model(bclasses, set_of, ia, ib) -> np.ndarray:
    """f64[N,4] for block rows [M,B,16]."""
    bclasses = np.asarray(bclasses)
    out = np.zeros((len(set_of), 4), np.float64)
    for t in range(len(set_of)):
        rows = bclasses[int(set_of[t])]
        out[t] = jackknife_row([int(v) for v in rows[:, int(ia[t])]], [int(v) for v in rows[:, int(ib[t])]])
    return out


def bits(x) -> np.ndarray:
    """f64 array -> its bit patterns (NaN compares equal to the same NaN)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def jackknife_case(N: int, B: int, seed: int = 0):
    """Designed input of the jackknife: block rows u32[M,B,16], set_of u32[N], ia / ib u8[N].  Test 0 holds counts of
    2^32 - 1 in every block, test 1 has a < b everywhere, test 2 has every block empty, test 3 exactly one non-empty
    block (g = 1), test 4 two non-empty blocks (only one when B = 1); the rest is random with empty blocks sprinkled in.
    The special tests own their set, so nobody else writes their slots."""
    rng = np.random.default_rng([seed, N, B])
    M = max(5, (N + 1) // 2)
    set_of = rng.integers(0, M, size=N).astype(np.uint32)
    for t in range(min(N, 5)):
        set_of[t] = t
    if N > 5:
        set_of[5:] = rng.integers(5, M, size=N - 5) if M > 5 else 0
    ia = rng.integers(0, 15, size=N).astype(np.uint8)
    ib = ((ia + rng.integers(1, 15, size=N)) % 15).astype(np.uint8)
    rows = rng.integers(0, 3000, size=(M, B, 16)).astype(np.uint32)
    rows[rng.random((M, B, 16)) < 0.1] = 0
    rows[rng.random((M, B)) < 0.15] = 0                       # blocks with m_j = 0 for every pair of classes
    big = rng.random((M, B, 16)) < 0.02
    rows[big] = rng.integers(2**31, 2**32, size=int(big.sum()), dtype=np.uint64).astype(np.uint32)
    special = {0: lambda j: (0xFFFFFFFF, 0xFFFFFFFF), 1: lambda j: (3 + j % 7, 0xFFFFFFF0 - j),
               2: lambda j: (0, 0), 3: lambda j: (11, 4) if j == B // 2 else (0, 0),
               4: lambda j: (17 + j, 5) if j in (0, B - 1) else (0, 0)}
    for t, f in special.items():
        if t >= N:
            break
        for j in range(B):
            rows[t, j, ia[t]], rows[t, j, ib[t]] = f(j)
    return rows, set_of, ia, ib
