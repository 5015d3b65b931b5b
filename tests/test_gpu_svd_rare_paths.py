"""GPU: the rare cases the singular-value kernels keep out of their hot loops, met by only some lanes of a wave.

* tq_bdsqr_kernel runs its rotation step unguarded and sends a wave through the guarded copy of a step when one of its
  sweeping lanes has a squared pivot below 1e-290.  Two families of bidiagonals stand among ordinary ones:
  - "tiny": ordinary bidiagonals scaled by 2^-500 (every squared pivot underflows the clamp) and by 2^-482 (the
    squared pivots straddle 1e-290, so the two copies of the step alternate inside one sweep).  These are the matrices
    that reach the guarded copy.  The clamp makes their values meaningless as singular values, in the parent as here,
    so the reference is what the parent commit's kernel gave, bit for bit (tests/golden/bdsqr_tiny_pivots.npz): the
    bare step gives other bits on them, so equality shows that the guarded copy ran.
  - "cancel": exact zeros on the diagonal, or d = 0 throughout.  The split search and the cancel branch remove these
    zeros before a sweep, so they never reach the guarded copy; they check that branch beside busy neighbours, against
    the 40-digit values.
  In both, every matrix must give bitwise what it gives in a wave of copies of itself: an ordinary lane that a
  neighbour drags through the guarded copy of a step keeps its bits.
* the bidiagonalisation kernels compute a reflector's coefficients without the "no reflector" selects and put the
  zeros in on a wave-uniform test: wave passes of 16 quartets that hold 1, 8 and 16 quartets with exactly zero rows
  and columns or low rank (designed_counts families (d) and (b)) among full-rank ones.
* tq_score_kernel runs blocks of 256 quartets: batch sizes around the block, a partial last wave, a single quartet.

The bars are those of tests/test_gpu_designed_svd.py: 1e-12 sigma_max against the 40-digit values, exact ranks, copies
bitwise equal.  Every test prints the worst value it saw before it asserts."""
from pathlib import Path

import numpy as np
import pytest

import designed_counts as D
import exact_ties as X
from test_gpu_designed_svd import Case

pytestmark = pytest.mark.gpu

SIGMA_BAR = X.ATOL_REL_SMAX          # 1e-12 sigma_max
WAVE = 64
NMATS = (1, 63, 64, 65, 129)
BIG = 33_000                         # >= 32 768 rows: the pass-loop form of the bidiagonalisation kernels
GOLDEN_TINY = Path(__file__).resolve().parent / "golden" / "bdsqr_tiny_pivots.npz"


# ---------------------------------------------------------------------------------------------------
# tq_bdsqr_kernel: squared pivots below the clamp, and the cancel family, in some lanes of a wave
# ---------------------------------------------------------------------------------------------------
def _ordinary_bidiagonals(seed, n=16):
    o = np.random.default_rng(seed).uniform(0.5, 2.0, size=(n, 32))
    o[:, 16] = 0.0
    return o


def tiny_pivot_bidiagonals():
    """f64[16, 32]: ordinary bidiagonals in [0.5, 2), eight scaled by 2^-500 (values ~3e-151: every f^2 + h^2 is below
    1e-290) and eight by 2^-482 (values 0.8e-145 .. 3.2e-145: squares 0.6e-290 .. 1e-289, on both sides of the clamp)."""
    t = _ordinary_bidiagonals(59)
    t[:8] *= 2.0 ** -500
    t[8:] *= 2.0 ** -482
    return t


def _cancel_bidiagonals():
    """(names, matrices with zeros on the diagonal, their twins with the zeros replaced by ones), f64[15, 32]: the
    unscaled designed cases with exact zeros on the diagonal or d = 0 throughout."""
    cases = D.bidiagonal_cases()
    cases = cases[:len(cases) // 2]
    zero = [(n, d, e) for n, _, d, e in cases if n.startswith("d zero at") or n == "d = 0, e live"]
    assert len(zero) == 15
    z = np.stack([np.concatenate([d, e]) for _, d, e in zero])
    twin = z.copy()
    twin[:, :16][z[:, :16] == 0] = 1.0
    return [n for n, _, _ in zero], z, twin


class Pool:
    """Rare matrices then ordinary ones, and what each gives alone in a wave of 64 copies of itself."""

    def __init__(self, eng, rare, ordinary):
        self.nrare, self.nord = len(rare), len(ordinary)
        self.de = np.concatenate([rare, ordinary])
        self.alone = []
        for i in range(len(self.de)):
            sv, st, sw, _ = eng.debug_bdsqr(np.repeat(self.de[i:i + 1], WAVE, axis=0), reps=1)
            assert (sv.view(np.uint64) == sv[0].view(np.uint64)).all() and (st == st[0]).all() and (sw == sw[0]).all(), \
                f"copies differ: matrix {i}"
            self.alone.append((sv[0], int(st[0]), int(sw[0])))


@pytest.fixture(scope="module")
def bdsqr():
    from tetrad_amd.engine import QuartetEngine
    names, z, twin = _cancel_bidiagonals()
    ordinary = _ordinary_bidiagonals(58)
    with QuartetEngine(0) as eng:
        pools = {"cancel": Pool(eng, z, ordinary), "tiny": Pool(eng, tiny_pivot_bidiagonals(), ordinary)}
        yield eng, names, twin, pools


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_tiny_pivot_matrices_give_the_bits_of_the_guarded_kernel(bdsqr):
    """The matrices whose squared pivots fall below 1e-290 give, alone in a wave of copies, bit for bit the values and
    the work counters that the kernel with the clamp and the selects in every step gave (the parent commit's, recorded
    by tests/golden/make_bdsqr_tiny_pivots.py).  The bare step alone cannot: where zz < 1e-290 it divides by the true
    root and not by the clamp's, so at least the first eight matrices would differ in every value."""
    eng, names, twin, pools = bdsqr
    pool = pools["tiny"]
    g = np.load(GOLDEN_TINY)
    np.testing.assert_array_equal(g["de"], pool.de[:pool.nrare], err_msg="the fixture was made from other matrices")
    bad = []
    for i in range(pool.nrare):
        sv, st, sw = pool.alone[i]
        print(f"[bdsqr tiny pivots] matrix {i}: {st} steps / {sw} sweeps, largest value {np.fmax.reduce(np.abs(sv)):.3e}, "
              f"not-converged sign {bool(np.signbit(sv).any())}")
        if not (_same_bits(sv, g["sv"][i]) and st == int(g["steps"][i]) and sw == int(g["sweeps"][i])):
            bad.append(i)
    assert not bad, f"matrices {bad} differ from the guarded kernel's values"
    assert int(g["steps"].min()) > 0, "a fixture matrix that runs no rotation step shows nothing"


def test_cancel_family_alone_reaches_the_40_digit_values(bdsqr):
    eng, names, twin, pools = bdsqr
    pool = pools["cancel"]
    worst = 0.0
    for i in range(len(pool.de)):
        ref = D.mp_bidiag_svd(pool.de[i, :16], pool.de[i, 16:])
        sv = pool.alone[i][0]
        assert np.isfinite(sv).all() and not np.signbit(sv).any(), f"matrix {i}: not-converged sign or non-finite value"
        err = float(np.abs(-np.sort(-sv) - ref).max() / ref[0])
        worst = max(worst, err)
        assert err <= SIGMA_BAR, f"matrix {i}: {err:.3e} sigma_max from the 40-digit values"
    print(f"[bdsqr cancel family] worst |sigma_dev - sigma_mp| / sigma_max = {worst:.3e} over {len(pool.de)} matrices")


def test_cancel_family_does_other_work_than_its_twins(bdsqr):
    """The work counters (rotation steps, sweeps) of a matrix with zeros on the diagonal differ from those of the same
    matrix with the zeros replaced by ones: the cancel branch and the splits it leaves were taken (this says nothing
    about the guarded copy of the rotation step, which these matrices do not reach)."""
    eng, names, twin, pools = bdsqr
    alone = pools["cancel"].alone
    _, st_t, sw_t, _ = eng.debug_bdsqr(twin, reps=1)
    for i, n in enumerate(names):
        print(f"[bdsqr cancel family] {n}: {alone[i][1]} steps / {alone[i][2]} sweeps, twin {st_t[i]} / {sw_t[i]}")
    same = [n for i, n in enumerate(names) if alone[i][1] == st_t[i] and alone[i][2] == sw_t[i]]
    assert not same, f"no trace of the zeros in the work counters of {same}"


def _rare_lanes(nmat, rng):
    """Positions 0, 31, 63 and one random lane of every wave, as far as the set reaches."""
    at = set()
    for w0 in range(0, nmat, WAVE):
        for lane in (0, 31, 63, int(rng.integers(WAVE))):
            if w0 + lane < nmat:
                at.add(w0 + lane)
    return sorted(at)


@pytest.mark.parametrize("nmat", NMATS)
@pytest.mark.parametrize("mix", ["some", "every", "none"])
@pytest.mark.parametrize("family", ["tiny", "cancel"])
def test_waves_with_rare_matrices_in_some_every_and_no_lane(bdsqr, family, nmat, mix):
    """Every matrix of the set, rare or ordinary, gives bitwise, values and work counters, what it gives in a wave of
    copies of itself.  With the tiny family the "some" waves take the guarded copy of a step because of four lanes and
    carry up to sixty ordinary matrices through it."""
    eng, names, twin, pools = bdsqr
    pool = pools[family]
    rng = np.random.default_rng([nmat, len(mix), len(family)])
    nr = pool.nrare
    if mix == "every":
        pick = (np.arange(nmat) + int(rng.integers(nr))) % nr
    else:
        pick = nr + rng.integers(pool.nord, size=nmat)
        if mix == "some":
            at = _rare_lanes(nmat, rng)
            pick[at] = rng.integers(nr, size=len(at))
    sv, st, sw, _ = eng.debug_bdsqr(pool.de[pick], reps=1)
    for j, i in enumerate(pick):
        assert _same_bits(sv[j], pool.alone[i][0]), f"{family} nmat={nmat} {mix}: matrix {i} at position {j}"
        assert (int(st[j]), int(sw[j])) == pool.alone[i][1:], f"{family} nmat={nmat} {mix}: work of matrix {i} at {j}"


# ---------------------------------------------------------------------------------------------------
# designed count matrices: dead reflectors in 1, 8 and 16 quads of a wave pass; the score kernel's block
# ---------------------------------------------------------------------------------------------------
def _ordinary_designs(n=4):
    """Dense full-rank matrices (counts 1..5 in every cell but the invariant ones): every reflector is live."""
    out = []
    seed = 0
    while len(out) < n:
        m = np.random.default_rng([9, seed]).integers(1, 6, size=(16, 16))
        for k in D.INVARIANT:
            m[k, k] = 0
        if int(X.exact_rank(m)) == 16:
            out.append(D.Design("o", f"dense seed={seed}", m, rank=16))
        seed += 1
    return out


def _pass_rows(n_ord, n_rare):
    """Batch rows as (design index, taxon order) in wave passes of 16 quartets that hold 1, 8 and 16 rare quartets in
    turn (the rare ones at the front, interleaved, everywhere), until every rare design stood in each kind of pass."""
    rows, r, o = [], 0, 0
    ident = (0, 1, 2, 3)
    for k in range(3 * n_rare):
        kind = (1, 8, 16)[k % 3]
        slots = {1: [0], 8: list(range(0, 16, 2)), 16: list(range(16))}[kind]
        for s in range(16):
            if s in slots:
                rows.append((n_ord + r % n_rare, ident))
                r += 1
            else:
                rows.append((o % n_ord, ident))
                o += 1
        if r >= 3 * n_rare and k % 3 == 2:
            break
    return rows


@pytest.fixture(scope="module")
def designed():
    """One data set of the dense designs and families (d) and (b); the batch in passes of 16; its rows resolved with
    debug outputs as they stand and tiled to 33 000 rows."""
    from tetrad_amd.engine import QuartetEngine
    ordinary = _ordinary_designs()
    rare = D.interleaved_designs() + D.exact_rank_designs(seeds=range(2))
    designs = ordinary + rare
    tmparr, tmpmap, quartets = D.realise(designs, seed=58)
    case = Case(designs, quartets, _pass_rows(len(ordinary), len(rare)))
    assert len(case.q) % 16 == 0 and len(case.q) < 32_768
    reps = -(-BIG // len(case.q))
    qbig = np.concatenate([case.q] * reps)[:BIG]
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        short = {sub: eng.resolve(case.q, sub, debug=True) for sub in (True, False)}
        big = eng.resolve(qbig, True, debug=True)
        yield eng, case, short, qbig, big


@pytest.mark.parametrize("sub", [True, False])
def test_passes_with_1_8_and_16_rank_deficient_quartets(designed, sub):
    """Ranks equal the exact ranks, singular values within 1e-12 sigma_max of the 40-digit ones, copies at other batch
    positions bitwise equal (Case.judge), in both modes."""
    eng, case, short, qbig, big = designed
    dead = int((case.ranks < 16).any(axis=1).sum())
    print(f"[rare reflectors] {len(case.q)} rows in passes of 16, {dead} with a rank-deficient flattening")
    case.judge(*short[sub], f"[passes of 1/8/16 rare quartets, sub={int(sub)}]")


def test_pass_loop_form_gives_the_rows_of_the_short_batch(designed):
    """33 000 rows take the loop-over-flattenings form of the bidiagonalisation kernel (the form of large batches): row
    for row and bit for bit what the short batch gave, whose rows the test above judges."""
    eng, case, short, qbig, big = designed
    rstat, rscor, flags, dbg = short[True]
    idx = np.arange(BIG) % len(case.q)
    for a, b, what in ((rstat, big[0], "rstat"), (rscor, big[1], "rscor"), (flags, big[2], "flags"),
                       (dbg["svds"], big[3]["svds"], "svds"), (dbg["ranks"], big[3]["ranks"], "ranks"),
                       (dbg["cmats"], big[3]["cmats"], "cmats")):
        np.testing.assert_array_equal(a[idx], b, err_msg=what)


@pytest.mark.parametrize("Q", [1, 255, 256, 257, 4125])
def test_score_rows_around_the_block_size(designed, Q):
    """Q quartets through `resolve` with debug outputs: a whole block, one lane more and less, a partial last wave and
    a single quartet give bitwise the same quartets' rows of the 33 000-row batch."""
    eng, case, short, qbig, big = designed
    off = 4099 if Q == 4125 else 0                   # not at a block boundary of the long batch
    got = eng.resolve(qbig[off:off + Q], True, debug=True)
    for a, b, what in ((got[0], big[0], "rstat"), (got[1], big[1], "rscor"), (got[2], big[2], "flags"),
                       (got[3]["svds"], big[3]["svds"], "svds"), (got[3]["ranks"], big[3]["ranks"], "ranks")):
        assert len(a) == Q
        np.testing.assert_array_equal(a, b[off:off + Q], err_msg=f"Q={Q}: {what}")
