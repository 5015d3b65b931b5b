"""Pure NumPy / Python model of the site-pattern classes and of the D accumulation.

It shares nothing with the library's pattern-to-class table: the class of a site is found from the raw rows of
`tmparr` by equality tests between the four positions, and the class numbers are the position of the resulting string
in the list the issue states.  Full mode counts every complete, non-invariant site.  Subsample mode follows the
reference rule as `oracle.chunk_to_matrices_py` restates it: a site is counted when it is unmasked and its locus differs
from the locus of the last counted site, i.e. the first complete, non-invariant site of each locus run.
"""
from __future__ import annotations

import numpy as np

STRINGS = ["0000", "0001", "0010", "0011", "0012", "0100", "0101", "0102", "0110", "0111", "0112", "0120", "0121", "0122",
           "0123"]
SIZES = [4, 12, 12, 12, 24, 12, 12, 24, 12, 12, 24, 24, 24, 24, 24]
CODE = {int(s, 4): i for i, s in enumerate(STRINGS)}


def site_classes(r: np.ndarray) -> np.ndarray:
    """r u8[4,S] (bases 0..3) -> class of every site, by equality tests between the positions."""
    e01, e02, e03 = r[0] == r[1], r[0] == r[2], r[0] == r[3]
    e12, e13, e23 = r[1] == r[2], r[1] == r[3], r[2] == r[3]
    l1 = np.where(e01, 0, 1)
    top = l1
    l2 = np.where(e02, 0, np.where(e12, l1, top + 1))
    top = np.maximum(top, l2)
    l3 = np.where(e03, 0, np.where(e13, l1, np.where(e23, l2, top + 1)))
    code = 16 * l1 + 4 * l2 + l3
    lut = np.full(64, -1, np.int64)
    for k, v in CODE.items():
        lut[k] = v
    out = lut[code]
    assert (out >= 0).all()
    return out


def counted_sites(rows: np.ndarray, locus: np.ndarray, subsample: bool, count_invariant: bool = False) -> np.ndarray:
    """Indices of the sites a quartet with these four rows counts."""
    masked = (rows > 3).any(axis=0)
    if not count_invariant:
        masked |= (rows == rows[0]).all(axis=0)
    idx = np.flatnonzero(~masked)
    if subsample and idx.size:
        loc = np.asarray(locus)[idx]
        idx = idx[np.concatenate([[True], loc[1:] != loc[:-1]])]
    return idx


def model_classes(tmparr, tmpmap, sets, subsample: bool, count_invariant: bool = False) -> np.ndarray:
    """u32[Q,16]: class counts and their sum for every row of `sets` (any order of the four taxa)."""
    tmparr = np.asarray(tmparr)
    tm = np.asarray(tmpmap)
    locus = tm[:, 0] if tm.ndim == 2 else tm
    sets = np.asarray(sets).reshape(-1, 4)
    out = np.zeros((sets.shape[0], 16), np.uint32)
    for i, q in enumerate(sets):
        rows = tmparr[q.astype(np.int64)]
        idx = counted_sites(rows, locus, subsample, count_invariant)
        c = np.bincount(site_classes(rows[:, idx]), minlength=15)
        out[i, :15] = c
        out[i, 15] = c.sum()
    return out


def table_classes(counts256: np.ndarray, table: np.ndarray) -> np.ndarray:
    """u32[Q,16] from count rows u[Q,256] (slab order 64 x0 + 16 x1 + 4 x2 + x3) and a pattern-to-class table."""
    counts256 = np.asarray(counts256).reshape(-1, 256).astype(np.int64)
    out = np.zeros((counts256.shape[0], 16), np.int64)
    for c in range(15):
        out[:, c] = counts256[:, np.asarray(table) == c].sum(axis=1)
    out[:, 15] = counts256.sum(axis=1)
    assert out.max(initial=0) < 2**32
    return out.astype(np.uint32)


def direct_abba_baba(tmparr, test):
    """(abba, baba) of a test (P1, P2, P3, O) counted from the rows in role order, full mode."""
    r = np.asarray(tmparr)[np.asarray(test, np.int64)]
    ok = (r <= 3).all(axis=0)
    abba = ok & (r[0] == r[3]) & (r[1] == r[2]) & (r[0] != r[1])
    baba = ok & (r[0] == r[2]) & (r[1] == r[3]) & (r[0] != r[1])
    return int(abba.sum()), int(baba.sum())


def dstat_model(replicates, set_of, ia, ib, acc=None):
    """The accumulation on Python floats: replicates = list of class arrays [M,16]; returns acc as a list of N
    [n, s1, s2, last] lists (continues `acc` when given)."""
    N = len(set_of)
    acc = [[0.0, 0.0, 0.0, 0.0] for _ in range(N)] if acc is None else acc
    for classes in replicates:
        for t in range(N):
            a = int(classes[int(set_of[t])][int(ia[t])])
            b = int(classes[int(set_of[t])][int(ib[t])])
            if a + b == 0:
                continue
            d = (a - b) / (a + b)
            p = d * d
            acc[t][0] = acc[t][0] + 1.0
            acc[t][1] = acc[t][1] + d
            acc[t][2] = acc[t][2] + p
            acc[t][3] = d
    return acc


def moments_model(D, acc):
    """(boot_n, boot_mean, boot_std, Z) per test on Python floats; NaN where a denominator is zero."""
    import math
    out = []
    for d, (n, s1, s2, _) in zip(D, acc):
        if n == 0:
            out.append((0, math.nan, math.nan, math.nan))
            continue
        mean = s1 / n
        std = math.sqrt(max(0.0, s2 / n - mean * mean))
        z = float(d) / std if std > 0 and not math.isnan(float(d)) else math.nan
        out.append((int(n), mean, std, z))
    return out


def dstat_case(N: int, seed: int = 0, nrep: int = 5):
    """Synthetic input of the accumulation: `nrep` class arrays u32[M,16], set_of u32[N], ia / ib u8[N].  Test 0 holds
    counts at 2^32 - 1, test 1 has a < b in every replicate, test 2 has a + b = 0 in every replicate and test 3 in
    some; the rest is random, with zeros sprinkled in."""
    rng = np.random.default_rng([seed, N])
    M = max(1, (N + 2) // 3)
    set_of = rng.integers(0, M, size=N).astype(np.uint32)
    ia = rng.integers(0, 15, size=N).astype(np.uint8)
    ib = ((ia + rng.integers(1, 15, size=N)) % 15).astype(np.uint8)
    for t in range(min(N, 4)):
        set_of[t] = t % M
    reps = []
    for k in range(nrep):
        c = rng.integers(0, 2000, size=(M, 16)).astype(np.uint32)
        c[rng.random((M, 16)) < 0.2] = 0
        big = rng.random((M, 16)) < 0.05
        c[big] = rng.integers(2**31, 2**32, size=int(big.sum()), dtype=np.uint64).astype(np.uint32)
        reps.append(c)
    special = [(0, 0xFFFFFFFF, 0xFFFFFFFF - 7), (1, 3, 0xFFFFFFFF), (2, 0, 0), (3, None, None)]
    for t, a, b in special:
        if t >= N:
            break
        # the special tests own their two slots of their row: nobody else may write them
        for k, c in enumerate(reps):
            if t == 3:
                a, b = (0, 0) if k % 2 == 0 else (17 + k, 5)
            c[set_of[t], ia[t]], c[set_of[t], ib[t]] = a, b
    return reps, set_of, ia, ib
