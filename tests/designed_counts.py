"""Designed count matrices (a plain helper module for the CPU and GPU tests of the singular-value path).

A quartet's count matrix is the table of the 256 site patterns of its four taxa, so ANY non-negative integer 16x16
matrix M whose four invariant cells (5k, 5k) are zero can be produced: write M[4a+b][4c+d] sites with the bases
(a, b, c, d) into four rows of ``tmparr``.  The two other flattenings follow from the first
(``oracle.chunk_to_matrices_py``).  The matrices are integer, so their exact ranks (``exact_ties.exact_rank``) and a
40-digit SVD (``mpmath.svd_r``) give a reference that shares no algorithm with the device or with LAPACK.

The families (``small_designs``) hold the shapes that break a shifted QR iteration or a Householder reduction and
that data simulated on trees almost never contain: exactly repeated singular values, exact zeros on the diagonal of
the bidiagonal, identical diagonal blocks, ranks exactly at the min(10, ...) cap of the score rule, strong grading.
"""
from __future__ import annotations

from itertools import permutations

import numpy as np

import exact_ties as X

INVARIANT = (0, 5, 10, 15)
MISSING = 78
PERMS = list(permutations(range(4)))


class Design:
    """One designed first flattening: ``m`` u32[16,16], its family letter, a name and what the family promises
    (``rank``: the exact rank of ``m``; ``equal``: how many non-zero singular values of ``m`` are all equal)."""
    __slots__ = ("family", "name", "m", "rank", "equal")

    def __init__(self, family, name, m, rank=None, equal=None):
        m = np.asarray(m)
        assert m.shape == (16, 16) and (m >= 0).all() and m.max() < 2 ** 32
        self.family, self.name, self.m, self.rank, self.equal = family, name, m.astype(np.uint32), rank, equal

    @property
    def sites(self) -> int:
        return int(self.m.sum(dtype=np.int64))

    def __repr__(self):
        return f"Design({self.family}:{self.name}, {self.sites} sites)"


# ---------------------------------------------------------------------------------------------------
# design -> data
# ---------------------------------------------------------------------------------------------------
def flattenings(m: np.ndarray, order=(0, 1, 2, 3)) -> np.ndarray:
    """The three count matrices u32[3,16,16] of the quartet (t[order[0]], .., t[order[3]]) when the taxa (t0..t3) carry
    the first flattening ``m``: the count tensor C[a,b,c,d] = m[4a+b][4c+d] with its axes permuted, then
    M0[4a+b][4c+d] = M1[4a+c][4b+d] = M2[4a+d][4b+c] = C[a,b,c,d] (resolve_quartets.py:68-72)."""
    c = np.asarray(m).reshape(4, 4, 4, 4).transpose(order)
    return np.stack([c.reshape(16, 16), c.transpose(0, 2, 1, 3).reshape(16, 16), c.transpose(0, 3, 1, 2).reshape(16, 16)])


def flattening_of_order(order) -> list[int]:
    """Which flattening of the quartet in design order each flattening of the reordered quartet is, up to row and
    column permutations and a transpose (none of which moves a singular value or the rank): flattening t pairs axis 0
    with axis 1 + t, and that pairing is all that matters."""
    kinds = {frozenset((0, 1)): 0, frozenset((2, 3)): 0, frozenset((0, 2)): 1, frozenset((1, 3)): 1,
             frozenset((0, 3)): 2, frozenset((1, 2)): 2}
    return [kinds[frozenset((order[0], order[1 + t]))] for t in range(3)]


def _check(designs):
    for i, d in enumerate(designs):
        m = d.m if isinstance(d, Design) else np.asarray(d)
        if m.shape != (16, 16):
            raise ValueError(f"design {i}: shape {m.shape}, not (16, 16)")
        if any(int(m[k, k]) != 0 for k in INVARIANT):
            raise ValueError(f"design {i}: an invariant cell (5k, 5k) is non-zero; such sites are never counted")
        yield m.astype(np.int64)


def _columns(m: np.ndarray, rng=None) -> np.ndarray:
    """u8[4, sum(m)]: m[4a+b][4c+d] sites with the bases (a, b, c, d), in cell order or shuffled by ``rng``."""
    cell = np.repeat(np.arange(256), m.reshape(-1))
    if rng is not None:
        cell = rng.permutation(cell)
    return np.stack([cell >> 6, (cell >> 4) & 3, (cell >> 2) & 3, cell & 3]).astype(np.uint8)


def _tmpmap(S: int) -> np.ndarray:
    tmpmap = np.empty((S, 2), np.uint32)
    tmpmap[:, 0] = tmpmap[:, 1] = np.arange(S, dtype=np.uint32)      # every site is its own locus
    return tmpmap


def realise(designs, pack=True, seed=None):
    """(tmparr u8[T,S], tmpmap u32[S,2], quartets u32[N,4]) whose quartet k has design k as its first flattening in
    subsample mode and in full mode alike (every site is its own locus).  Design k owns taxa 4k..4k+3 and its own run of
    sites; at every other design's sites those four taxa are missing (78).  ``pack=False`` gives every design a data
    set of its own instead (T = 4): a list of such triples.  ``seed`` shuffles the sites inside each run.  Designs with
    a non-zero invariant cell are rejected."""
    mats = list(_check(designs))
    rng = None if seed is None else np.random.default_rng(seed)
    if not pack:
        out = []
        for m in mats:
            cols = _columns(m, rng)
            out.append((cols, _tmpmap(cols.shape[1]), np.arange(4, dtype=np.uint32)[None]))
        return out
    n = [int(m.sum()) for m in mats]
    tmparr = np.full((4 * len(mats), sum(n)), MISSING, np.uint8)
    o = 0
    for k, m in enumerate(mats):
        tmparr[4 * k:4 * k + 4, o:o + n[k]] = _columns(m, rng)
        o += n[k]
    quartets = np.arange(4 * len(mats), dtype=np.uint32).reshape(-1, 4)
    return tmparr, _tmpmap(sum(n)), quartets


def concentrated(S: int, patterns=((0, 1, 2, 3),)):
    """(tmparr u8[4,S], tmpmap, quartets, design): all S sites of four taxa carry the given patterns in turn (site i has
    patterns[i % len]) -- the largest count a single cell can reach, the case the 16-bit bank-private counters of the
    scan are sized for."""
    pat = np.asarray(patterns, np.uint8)
    tmparr = np.ascontiguousarray(pat[np.arange(S) % len(pat)].T)
    m = np.zeros((16, 16), np.int64)
    for j, (a, b, c, d) in enumerate(patterns):
        m[4 * a + b, 4 * c + d] += len(range(j, S, len(pat)))
    return tmparr, _tmpmap(S), np.arange(4, dtype=np.uint32)[None], Design("z", f"concentrated S={S} x{len(pat)}", m)


# ---------------------------------------------------------------------------------------------------
# the 40-digit reference
# ---------------------------------------------------------------------------------------------------
_MP_CACHE: dict[bytes, np.ndarray] = {}


def mp_svd(m) -> np.ndarray:
    """Singular values f64[n] (descending) of a real matrix from mpmath's SVD at exact_ties.MP_DIGITS digits; cached by
    content for the session."""
    import mpmath
    a = np.ascontiguousarray(m)
    key = a.dtype.str.encode() + bytes(a.shape) + a.tobytes()
    got = _MP_CACHE.get(key)
    if got is None:
        with mpmath.workdps(X.MP_DIGITS):
            rows = [[mpmath.mpf(int(x)) if a.dtype.kind in "iu" else mpmath.mpf(float(x)) for x in r] for r in a]
            s = mpmath.svd_r(mpmath.matrix(rows), compute_uv=False)
            got = np.array(sorted((float(s[i]) for i in range(len(s))), reverse=True))
        _MP_CACHE[key] = got
    return got


def mp_bidiag_svd(d, e) -> np.ndarray:
    """40-digit singular values of the upper bidiagonal with diagonal d[0..n-1] and superdiagonal e[1..n-1] (e[i]
    couples columns i-1 and i; e[0] is not part of the matrix), the layout of the device's ``de`` scratch."""
    d, e = np.asarray(d, np.float64), np.asarray(e, np.float64)
    b = np.diag(d)
    b[np.arange(len(d) - 1), np.arange(1, len(d))] = e[1:]
    return mp_svd(b)


def mp_reference(cmats3):
    """(svds f64[3,16] descending, exact ranks i32[3], scores f64[3]) of one quartet's three integer count matrices:
    40-digit singular values, ranks by exact elimination, and the scores of resolve_quartets.py:243-251 with those
    ranks -- the norm of the singular values from index min(10, min rank) on, summed in 40 digits too."""
    import mpmath
    cm = np.asarray(cmats3).astype(np.int64)
    svds = np.stack([mp_svd(cm[t]) for t in range(3)])
    ranks = X.exact_rank(cm).astype(np.int32)
    minrank = min(10, int(ranks.min()))
    scores = np.zeros(3)
    with mpmath.workdps(X.MP_DIGITS):
        for t in range(3):
            # below the exact rank the exact singular values are zero; what the 40-digit SVD leaves there is its rounding
            tail = [mpmath.mpf(float(x)) for x in svds[t, minrank:int(ranks[t])]]
            scores[t] = float(mpmath.sqrt(mpmath.fsum(x * x for x in tail)))
    svds = np.where(np.arange(16)[None, :] < ranks[:, None], svds, 0.0)
    return svds, ranks, scores


def reorder_reference(ref, order):
    """The reference of the quartet with its taxa in ``order``, from the reference ``ref`` of the design order."""
    svds, ranks, scores = ref
    kind = flattening_of_order(order)
    return svds[kind], ranks[kind], scores[kind]


# ---------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------
def _clear_invariant(m):
    m = np.array(m, dtype=np.int64)
    for k in INVARIANT:
        m[k, k] = 0
    return m


def partial_permutation(k: int, c: int) -> Design:
    """(a) k cells of a cyclically shifted diagonal hold c: k singular values equal to c, the others zero."""
    shift = 1 + (7 * k) % 15
    m = np.zeros((16, 16), np.int64)
    rows = (np.arange(k) * 5) % 16                    # 5 is a unit mod 16: k distinct rows, spread over the matrix
    m[rows, (rows + shift) % 16] = c
    return Design("a", f"perm k={k} c={c}", m, rank=k, equal=k)


def _rank_r(r: int, rng, density=0.35):
    """A sum of r outer products of sparse 0/1 vectors with exact rank r and no count in an invariant cell (the
    vectors of even terms vanish on rows 0/5/10/15, those of odd terms on the columns)."""
    inv = list(INVARIANT)
    while True:
        m = np.zeros((16, 16), np.int64)
        for j in range(r):
            u = (rng.random(16) < density).astype(np.int64)
            v = (rng.random(16) < density).astype(np.int64)
            (u if j % 2 == 0 else v)[inv] = 0
            if not u.any():
                u[1 + j % 4] = 1
            if not v.any():
                v[1 + j % 4] = 1
            m += np.outer(u, v)
        if int(X.exact_rank(m)) == r:
            return m


def exact_rank_designs(seeds=range(8)):
    """(b) exact rank r = 1..16."""
    out = []
    for r in range(1, 17):
        for s in seeds:
            rng = np.random.default_rng([2, r, s])
            out.append(Design("b", f"rank r={r} seed={s}", _rank_r(r, rng, 0.35 if r < 14 else 0.5), rank=r))
    return out


def block_designs(seeds=range(5)):
    """(c) nb identical bs x bs blocks on a block diagonal shifted by one block column (a column permutation of the
    block diagonal, which keeps the invariant cells free): every singular value of the block occurs nb times.  The
    same with +1 in one cell of the first block: near-repeated clusters."""
    out = []
    for bs, nbs in ((4, (2, 3, 4)), (8, (2,))):
        for nb in nbs:
            for s in seeds:
                rng = np.random.default_rng([3, bs, nb, s])
                while True:
                    blk = rng.integers(0, 5 if bs == 4 else 4, size=(bs, bs))
                    if int(X.exact_rank(blk)) == bs:
                        break
                m = np.zeros((16, 16), np.int64)
                nslot = 16 // bs
                for i in range(nb):
                    j = (i + 1) % nslot
                    m[bs * i:bs * i + bs, bs * j:bs * j + bs] = blk
                out.append(Design("c", f"blocks {nb}x{bs} seed={s}", m, rank=nb * bs, equal=nb))
                m1 = m.copy()
                m1[int(rng.integers(bs)), bs + int(rng.integers(bs))] += 1
                out.append(Design("c+", f"blocks {nb}x{bs} seed={s} +1", m1))
    return out


def interleaved_designs(seeds=range(3)):
    """(d) live rows and columns interleaved with zero ones."""
    out = []
    for s in seeds:
        rng = np.random.default_rng([4, s])
        full = rng.integers(1, 6, size=(16, 16))
        rows = np.zeros(16, bool)
        rows[[1, 6, 11, 12]] = True
        even = np.arange(16) % 2 == 0
        for name, rm, cm in (("rows 1,6,11,12", rows, np.ones(16, bool)), ("every second column", np.ones(16, bool), even),
                             ("every second row", ~even, np.ones(16, bool)), ("rows 1,6,11,12 x even columns", rows, even),
                             ("odd rows x even columns", ~even, even), ("one row", np.arange(16) == 6, np.ones(16, bool)),
                             ("one column", np.ones(16, bool), np.arange(16) == 9),
                             ("one cell", np.arange(16) == 3 + s, np.arange(16) == 12 - s)):
            m = _clear_invariant(full * rm[:, None] * cm[None, :])
            out.append(Design("d", f"{name} seed={s}", m))
    return out


def graded(top: int, bottom: int, how: str, seed: int) -> Design:
    """(e) a cyclically shifted diagonal 2^top, 2^(top-1), .., 2^bottom (the rest of the diagonal stays empty when
    fewer than 16 powers are asked for) plus 0/1 noise everywhere; ``how``: the powers top-down ("down"), bottom-up
    ("up") or shuffled."""
    rng = np.random.default_rng([5, top, bottom, seed])
    p = 2 ** np.arange(top, bottom - 1, -1, dtype=np.int64)
    if how == "up":
        p = p[::-1]
    elif how == "shuffled":
        p = rng.permutation(p)
    m = (rng.random((16, 16)) < 0.5).astype(np.int64)
    r = np.arange(len(p))
    m[r, (r + 3) % 16] += p
    return Design("e", f"graded 2^{top}..2^{bottom} {how} seed={seed}", _clear_invariant(m))


def near_deficient_designs(seeds=range(3)):
    """(f) an exact rank-r design plus 1 in one cell."""
    out = []
    for r in range(1, 16):
        for s in seeds:
            rng = np.random.default_rng([6, r, s])
            m = _rank_r(r, rng)
            while True:
                i, j = (int(x) for x in rng.integers(16, size=2))
                if not (i == j and i in INVARIANT):
                    break
            m[i, j] += 1
            out.append(Design("f", f"rank r={r} seed={s} +1 at ({i},{j})", m))
    return out


_SMALL = None


def small_designs() -> list[Design]:
    """The small designs of all families (about 300, a few hundred sites each): realised together into one data set."""
    global _SMALL
    if _SMALL is None:
        out = [partial_permutation(k, c) for c in (1, 3) for k in range(1, 17)]
        out += exact_rank_designs()
        out += block_designs()
        out += interleaved_designs()
        out += [graded(10, 0, how, s) for how in ("down", "up", "shuffled") for s in (0, 1)]
        out += near_deficient_designs()
        _SMALL = out
    return list(_SMALL)


def large_designs() -> list[Design]:
    """Designs with too many sites to share a data set: (a) with c = 50 000 at every k, and (e) at full size (six
    decades: 2^20 .. 2^5).  Their matrices take part in every CPU check of the reference machinery."""
    return [partial_permutation(k, 50_000) for k in range(1, 17)] + \
           [graded(20, 5, how, 0) for how in ("down", "up", "shuffled")]


def big_designs() -> list[Design]:
    """The large designs that the GPU test realises, each in its own 4-taxon data set."""
    return [d for d in large_designs() if d.family == "e" or d.name == "perm k=16 c=50000"]


# ---------------------------------------------------------------------------------------------------
# bidiagonals that count matrices cannot reach (tq_bdsqr_kernel alone)
# ---------------------------------------------------------------------------------------------------
def bidiagonal_cases():
    """[(name, kind, d f64[16], e f64[16])] with e[0] = 0; ``kind`` "cancel" marks the cases with an exact zero on the
    diagonal above a live superdiagonal.  Every case comes a second time scaled by 2^32 (exact in f64)."""
    rng = np.random.default_rng(7)
    one = np.ones(16)
    cases = []

    def add(name, kind, d, e):
        d, e = np.array(d, np.float64), np.array(e, np.float64)
        e[0] = 0.0
        cases.append((name, kind, d, e))

    add("toeplitz d=e=1", "plain", one, one)
    add("d=2^-i e=1", "plain", 2.0 ** -np.arange(16), one)
    add("d=2^-(15-i) e=1", "plain", 2.0 ** -np.arange(15, -1, -1.0), one)
    for zeros in ((0,), (7,), (15,), (0, 7), (3, 4), (7, 15), (0, 15)):
        for base in ("ones", "random"):
            d = one.copy() if base == "ones" else rng.uniform(0.5, 2.0, 16)
            e = one.copy() if base == "ones" else rng.uniform(0.5, 2.0, 16)
            d[list(zeros)] = 0.0
            add(f"d zero at {zeros} ({base})", "cancel" if min(zeros) < 15 else "plain", d, e)
    d0, e0 = rng.uniform(0.5, 2.0, 16), rng.uniform(0.5, 2.0, 16)
    for i in range(1, 16):
        e = e0.copy()
        e[i] = 0.0
        add(f"e zero at {i}", "split", d0, e)
    for i, j in ((1, 2), (1, 15), (4, 9), (7, 8), (8, 12), (2, 14), (14, 15), (5, 6)):
        e = e0.copy()
        e[[i, j]] = 0.0
        add(f"e zero at {i},{j}", "split", d0, e)
    add("e = 0, some d negative", "plain", d0 * np.where(np.arange(16) % 3 == 1, -1.0, 1.0), np.zeros(16))
    add("d = 0, e live", "cancel", np.zeros(16), e0)
    add("all zero", "plain", np.zeros(16), np.zeros(16))
    for i in (0, 9, 15):
        d = np.zeros(16)
        d[i] = 3.0
        add(f"only d[{i}]", "plain", d, np.zeros(16))
    for i in (1, 8, 15):
        e = np.zeros(16)
        e[i] = 3.0
        add(f"only e[{i}]", "cancel", np.zeros(16), e)
    add("cluster d=1+j 2^-40, e=2^-20", "plain", 1.0 + np.arange(16) * 2.0 ** -40, one * 2.0 ** -20)
    add("cluster d=1+j 2^-40, e=1", "plain", 1.0 + np.arange(16) * 2.0 ** -40, one)
    add("cluster d=1+j 2^-40, e=0", "plain", 1.0 + np.arange(16) * 2.0 ** -40, np.zeros(16))
    return cases + [(f"{n} x 2^32", k, d * 2.0 ** 32, e * 2.0 ** 32) for n, k, d, e in cases]
