"""Exact adjudication of tied and near-tied quartet rows (a plain helper module for the GPU tests).

resolve_quartets.py:243-251 scores flattening t as the norm of its singular values from index
``minrank = min(10, min_t rank_t)`` on.  The ranks of integer count matrices can be computed exactly, and
with them the scores that are exactly zero: score t == 0 iff rank_t == minrank.  Z is that set of
flattenings.  |Z| >= 2 is an exact tie (any member is a correct topology, and the device must flag the
row); |Z| == 1 decides the argmin whatever the rounding of the SVD.  Only when Z is empty (every rank
above 10) do rows whose two lowest scores are within rounding of each other need an extended-precision
SVD (``mp_scores``).
"""
from __future__ import annotations

import numpy as np

RTOL = 1e-6
ATOL_REL_SMAX = 1e-12
FLAG_GAP = 1e-9          # the device's and the oracle's TQ_FLAG_DEGENERATE threshold, relative to sigma_max
MP_DIGITS = 40


def _rank_one(m: np.ndarray) -> int:
    """Rank of one integer matrix: fraction-free Gaussian (Bareiss) elimination over Python ints."""
    m = m[m.any(axis=1)][:, m.any(axis=0)]            # zero rows and columns do not count
    if m.size == 0:
        return 0
    a = [[int(x) for x in row] for row in m.tolist()]
    rows, cols = len(a), len(a[0])
    rank, prev, r = 0, 1, 0
    for c in range(cols):
        piv = next((i for i in range(r, rows) if a[i][c]), None)
        if piv is None:
            continue
        a[r], a[piv] = a[piv], a[r]
        p = a[r][c]
        for i in range(r + 1, rows):
            ai = a[i]
            f = ai[c]
            ar = a[r]
            for j in range(c + 1, cols):
                ai[j] = (p * ai[j] - f * ar[j]) // prev
            ai[c] = 0
        prev = p
        r += 1
        rank += 1
        if r == rows:
            break
    return rank


_P = 2147483629          # a prime below 2^31: products of two residues fit in int64


def _rank_mod_p(a: np.ndarray) -> np.ndarray:
    """Ranks over GF(_P) of integer matrices [N, n, m] (fraction-free elimination, vectorised over N).  A lower
    bound of the rank over the rationals."""
    a = np.asarray(a, dtype=np.int64) % _P
    N, R, C = a.shape
    ar = np.arange(N)
    used = np.zeros((N, R), bool)
    rank = np.zeros(N, np.int32)
    for c in range(C):
        cand = (a[:, :, c] != 0) & ~used
        has = cand.any(axis=1)
        piv = np.argmax(cand, axis=1)
        prow = a[ar, piv]
        elim = ~used & has[:, None]
        elim[ar, piv] = False
        new = (prow[:, c, None, None] * a - a[:, :, c, None] * prow[:, None, :]) % _P
        a = np.where(elim[:, :, None], new, a)
        used[ar[has], piv[has]] = True
        rank += has
    return rank


def exact_rank(cmats: np.ndarray) -> np.ndarray:
    """Exact ranks of integer matrices [..., n, m] -> int32 [...].  The rank modulo a prime is a lower bound;
    where it reaches min(nonzero rows, nonzero columns) it is the rank, elsewhere Bareiss decides."""
    cmats = np.asarray(cmats)
    flat = cmats.reshape(-1, *cmats.shape[-2:])
    out = _rank_mod_p(flat)
    bound = np.minimum(flat.any(axis=2).sum(axis=1), flat.any(axis=1).sum(axis=1))
    for i in np.flatnonzero(out != bound):
        out[i] = _rank_one(flat[i])
    return out.reshape(cmats.shape[:-2])


def zero_tail_set(ranks) -> set[int]:
    """Z: the flattenings whose score is exactly zero, from the exact ranks r_t of the three flattenings."""
    r = [int(x) for x in ranks]
    minrank = min(10, min(r))
    return {t for t in range(3) if r[t] == minrank}


def mp_scores(cmat3: np.ndarray, minrank: int) -> np.ndarray:
    """The three scores of one quartet from a 40-digit SVD of its count matrices (float64 of the result)."""
    import mpmath
    out = np.zeros(3)
    with mpmath.workdps(MP_DIGITS):
        for t in range(3):
            s = mpmath.svd_r(mpmath.matrix(cmat3[t].astype(np.int64).tolist()), compute_uv=False)
            s = sorted((s[i] for i in range(len(s))), reverse=True)
            out[t] = float(mpmath.sqrt(mpmath.fsum(x * x for x in s[minrank:])))
    return out


def _close(x, ref, smax, what):
    tol = RTOL * np.abs(ref) + ATOL_REL_SMAX * smax
    bad = np.abs(x - ref) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} values out of tolerance, worst {np.abs(x - ref).max()}"


def check_rows(dev, dbg, orc, exact=None):
    """The exact bar for every row.  ``dev`` = (rstat, rscor, flags) of the device, ``dbg`` its debug dict
    (cmats, svds, ranks), ``orc`` = (rstat, rscor, debug dict) of the oracle; ``exact`` the exact ranks
    [Q,3] if already known.  Returns the counts of the row kinds it judged."""
    rstat, rscor, flags = dev
    o_rstat, o_rscor, o = orc
    cm = o["cmats"]
    np.testing.assert_array_equal(dbg["cmats"], cm, err_msg="count matrices")
    np.testing.assert_array_equal(rstat[:, 1], o_rstat[:, 1], err_msg="nsnps")
    zero = o_rstat[:, 1] == 0
    np.testing.assert_array_equal((flags & 1) != 0, zero, err_msg="zero-data flag")
    assert (flags[zero] == 1).all() and (rstat[zero, 0] == 0).all() and (rscor[zero] == 0.001).all(), "zero-data rows"
    assert ((flags & 8) == 0).all(), "singular-value iteration hit its sweep cap"
    live = ~zero
    if exact is None:
        exact = np.zeros((len(cm), 3), np.int32)
        exact[live] = exact_rank(cm[live])
    np.testing.assert_array_equal(o["rank"][live], exact[live], err_msg="oracle (numpy) rank != exact rank")
    np.testing.assert_array_equal(dbg["ranks"][live], exact[live], err_msg="device rank != exact rank")
    smax = np.maximum(o["svds"].max(axis=(1, 2)), 1e-300)
    _close(dbg["svds"][live], o["svds"][live], smax[live, None, None], "singular values")
    _close(rscor[live], o_rscor[live], smax[live, None], "scores")
    n = dict(rows=len(cm), zero=int(zero.sum()))
    n.update(check_topology(np.flatnonzero(live), exact, cm, rstat[:, 0], (flags & 2) != 0, o_rscor, o_rstat[:, 0], smax))
    return n


def check_topology(rows, exact, cmats, topo, deg, ref_rscor, ref_topo, smax):
    """The topology and flag rules on the given rows (nsnps > 0), from the exact ranks [Q,3]: an exact tie Z
    (|Z| >= 2) must be flagged and answered inside Z, a lone zero score must be the answer unless the next score
    is within twice the flag threshold of it (40-digit SVD), and rows without zero scores must agree with the
    reference wherever its gap is decided, and lie in the 40-digit near-minimum set where it is not."""
    s = np.sort(ref_rscor, axis=1)
    ref_gap = s[:, 1] - s[:, 0]
    n = dict(tie=0, one=0, one_flagged=0, lowrank=0, empty=0, mp=0)
    for i in rows:
        ranks = exact[i].tolist()
        minrank = min(10, min(ranks))
        n["lowrank"] += minrank < 10
        Z = zero_tail_set(ranks)
        if len(Z) >= 2:
            n["tie"] += 1
            assert topo[i] in Z, f"row {i}: topology {topo[i]} outside the exact tie {sorted(Z)} (ranks {ranks})"
            assert deg[i], f"row {i}: exact tie {sorted(Z)} (ranks {ranks}) not flagged"
        elif len(Z) == 1:
            n["one"] += 1
            (z,) = Z
            if not deg[i]:
                assert topo[i] == z, f"row {i}: topology {topo[i]}, the only zero score is {z} (ranks {ranks})"
            else:
                n["one_flagged"] += 1
                n["mp"] += 1
                second = np.sort(mp_scores(cmats[i], minrank))[1]
                assert second <= 2 * FLAG_GAP * smax[i], \
                    f"row {i}: flagged, but the next score is {second / smax[i]:.2e} sigma_max above the only zero one {z}"
        else:
            n["empty"] += 1
            if ref_gap[i] > 2 * FLAG_GAP * smax[i]:
                assert topo[i] == ref_topo[i], f"row {i}: topology {topo[i]} != reference {ref_topo[i]}"
                assert not deg[i], f"row {i}: flagged, reference scores {ref_gap[i] / smax[i]:.2e} sigma_max apart"
            else:
                n["mp"] += 1
                mp = mp_scores(cmats[i], minrank)
                near = np.flatnonzero(mp - mp.min() <= FLAG_GAP * smax[i])
                assert topo[i] in near, f"row {i}: topology {topo[i]} outside the exact near-minimum set {near.tolist()}"
    return n
