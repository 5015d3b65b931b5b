"""GPU: the singular-value path (tq_bidiag_kernel / tq_bidiag2_kernel -> tq_bdsqr_kernel -> tq_score_kernel, and the
Jacobi kernel) on DESIGNED count matrices against an exact reference -- exact ranks and a 40-digit SVD
(tests/designed_counts.py; tests/test_designed_counts_cpu.py pins the inputs and the reference machinery).

The bar for a singular value is |sigma_dev - sigma_mp| <= 1e-12 sigma_max of its matrix (exact_ties.ATOL_REL_SMAX
without the 1e-6 |ref| allowance of the general bar); for the bidiagonalisation alone 1e-13 sigma_max.  Every test
prints the worst value it saw before it asserts (run with -s to read them; DESIGN.md section 5 quotes them)."""
import numpy as np
import pytest

import designed_counts as D
import exact_ties as X

pytestmark = pytest.mark.gpu

SIGMA_BAR = X.ATOL_REL_SMAX          # 1e-12 sigma_max
BIDIAG_BAR = 1e-13                   # sigma(bidiagonal) vs sigma(integer matrix), relative to sigma_max
SVD_CONFIGS = (("hqr, 2x2 layout", 1, 1), ("hqr, column layout", 1, 0), ("jacobi", 0, 1))
NONZERO_ORDERS = [p for p in D.PERMS if p != (0, 1, 2, 3)]


def _configure(eng, svd_method, bidiag_layout):
    eng.set_option("svd_method", svd_method)
    eng.set_option("bidiag_layout", bidiag_layout)


class Case:
    """A batch of quartets over realised designs with the exact answer of every row."""

    def __init__(self, designs, quartets, rows):
        """``rows``: [(design index, taxon order)] per batch row; ``quartets``: the design quartets u32[N,4]."""
        self.design = np.array([i for i, _ in rows])
        self.order = [p for _, p in rows]
        self.q = np.stack([quartets[i][list(p)] for i, p in rows]).astype(np.uint32)
        base = {}
        for i in set(self.design.tolist()):
            cm = D.flattenings(designs[i].m)
            base[i] = (cm, D.mp_reference(cm))
        uniq = {}
        self.key = np.zeros(len(rows), np.int64)                     # rows with the same key are the same quartet
        for n, (i, p) in enumerate(rows):
            if (i, p) not in uniq:
                uniq[(i, p)] = (len(uniq), D.flattenings(designs[i].m, p), D.reorder_reference(base[i][1], p))
            self.key[n] = uniq[(i, p)][0]
        vals = sorted(uniq.values(), key=lambda v: v[0])
        self.cmats = np.stack([v[1] for v in vals])[self.key].astype(np.uint32)
        self.svds = np.stack([v[2][0] for v in vals])[self.key]
        self.ranks = np.stack([v[2][1] for v in vals])[self.key].astype(np.int32)
        self.scores = np.stack([v[2][2] for v in vals])[self.key]
        self.nsnps = np.array([designs[i].sites for i in self.design])
        self.first = np.zeros(len(rows), np.int64)                   # first row of each row's key
        seen = {}
        for n, k in enumerate(self.key.tolist()):
            self.first[n] = seen.setdefault(k, n)

    def prefix(self, n):
        c = object.__new__(Case)
        for name in ("design", "q", "key", "cmats", "svds", "ranks", "scores", "nsnps"):
            setattr(c, name, getattr(self, name)[:n])
        c.order = self.order[:n]
        c.first = self.first[:n]                                      # first occurrences never lie behind a row
        return c

    def judge(self, rstat, rscor, flags, dbg, what):
        """Every assertion of one configuration; returns the worst |sigma_dev - sigma_mp| / sigma_max."""
        np.testing.assert_array_equal(dbg["cmats"], self.cmats, err_msg=f"{what}: count matrices != design")
        np.testing.assert_array_equal(rstat[:, 1], self.nsnps, err_msg=f"{what}: nsnps")
        assert ((flags & 8) == 0).all(), f"{what}: {int(((flags & 8) != 0).sum())} rows hit the sweep cap"
        assert ((flags & ~np.uint8(2)) == 0).all(), f"{what}: unexpected flags {np.unique(flags)}"
        smax_m = self.svds[:, :, :1]                                   # of each matrix
        smax_q = self.svds.max(axis=(1, 2))                            # of each quartet
        err = np.abs(dbg["svds"] - self.svds) / smax_m
        worst = float(err.max())
        w = np.unravel_index(np.argmax(err), err.shape)
        print(f"{what}: worst |sigma_dev - sigma_mp| / sigma_max = {worst:.3e} (row {w[0]}, flattening {w[1]}, value {w[2]}; "
              f"{len(self.q)} quartets)")
        serr = np.abs(rscor - self.scores)
        print(f"{what}: worst score error {float((serr / smax_q[:, None]).max()):.3e} sigma_max")
        np.testing.assert_array_equal(dbg["ranks"], self.ranks, err_msg=f"{what}: device rank != exact rank")
        assert worst <= SIGMA_BAR, f"{what}: singular value {worst:.3e} sigma_max away from the 40-digit value"
        assert (serr <= X.RTOL * np.abs(self.scores) + X.ATOL_REL_SMAX * smax_q[:, None]).all(), f"{what}: scores"
        # position independence: the copies of a quartet at other batch positions are bitwise the first one
        for name, a in (("svds", dbg["svds"]), ("rscor", rscor), ("rstat", rstat)):
            np.testing.assert_array_equal(a, a[self.first], err_msg=f"{what}: {name} depends on the batch position")
        # topology and the noise flag, judged exactly; once per distinct quartet (the copies are bitwise equal)
        rows = np.unique(self.first)
        n = X.check_topology(rows, self.ranks, self.cmats, rstat[:, 0], (flags & 2) != 0, self.scores,
                             np.argmin(self.scores, axis=1), smax_q)
        print(f"{what}: topology rows {n}")
        return worst, n


@pytest.fixture(scope="module")
def small():
    designs = D.small_designs()
    tmparr, tmpmap, quartets = D.realise(designs, seed=11)
    rng = np.random.default_rng(2024)
    rows = []
    for i in range(len(designs)):
        rows += [(i, (0, 1, 2, 3))] * 3                                # three copies at different batch positions
        rows += [(i, NONZERO_ORDERS[j]) for j in rng.choice(len(NONZERO_ORDERS), size=12, replace=False)]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    assert len(rows) >= 4096
    return designs, tmparr, tmpmap, quartets, Case(designs, quartets, rows)


@pytest.fixture(scope="module")
def engine(small):
    from tetrad_amd.engine import QuartetEngine
    eng = QuartetEngine(0)
    eng.set_data(small[1], small[2])
    yield eng
    eng.close()


@pytest.mark.parametrize("name,svd_method,bidiag_layout", SVD_CONFIGS)
def test_designed_batch_against_the_exact_reference(engine, small, name, svd_method, bidiag_layout):
    """All small designs in one data set; a shuffled batch of every design's quartet three times plus twelve other
    taxon orders each (>= 4 096 rows), and a prefix of 900 rows, in both modes."""
    case = small[4]
    _configure(engine, svd_method, bidiag_layout)
    try:
        kinds = None
        for sub in (True, False):
            for c, tag in ((case, "batch"), (case.prefix(900), "prefix")):
                got = engine.resolve(c.q, sub, debug=True)
                _, n = c.judge(*got, f"[{name}, sub={int(sub)}, {tag}]")
                kinds = n if tag == "batch" else kinds
        # the batch really holds what the topology rules are written for
        assert kinds["tie"] >= 100 and kinds["one"] >= 100 and kinds["empty"] >= 100 and kinds["lowrank"] >= 100, kinds
    finally:
        _configure(engine, 1, 1)


@pytest.mark.parametrize("name,svd_method,bidiag_layout", SVD_CONFIGS[:2])
def test_designed_batch_in_the_pass_loop_form(engine, small, name, svd_method, bidiag_layout):
    """A singular-value chunk of 32 768 quartets or more takes the other form of the bidiagonalisation kernels (a loop
    over the three flattenings inside one block instead of one block per flattening): the batch tiled to 33 000 rows
    must give, row for row and bit for bit, what the short batch gave, whose rows the test above judges."""
    case = small[4]
    reps = -(-32_768 // len(case.q))
    q = np.concatenate([case.q] * reps)
    assert len(q) >= 32_768
    _configure(engine, svd_method, bidiag_layout)
    try:
        for sub in (True, False):
            rstat, rscor, flags, dbg = engine.resolve(case.q, sub, debug=True)
            worst, _ = case.judge(rstat, rscor, flags, dbg, f"[{name}, sub={int(sub)}, short]")
            big = engine.resolve(q, sub, debug=True)
            for a, b, what in ((rstat, big[0], "rstat"), (rscor, big[1], "rscor"), (flags, big[2], "flags"),
                               (dbg["svds"], big[3]["svds"], "svds"), (dbg["ranks"], big[3]["ranks"], "ranks"),
                               (dbg["cmats"], big[3]["cmats"], "cmats")):
                np.testing.assert_array_equal(np.concatenate([a] * reps), b, err_msg=f"{name} sub={sub}: {what}")
    finally:
        _configure(engine, 1, 1)


@pytest.mark.parametrize("name,bidiag_layout,step", [("2x2 layout", 1, 1), ("column layout", 0, 3)])
def test_bidiagonalisation_alone(engine, small, name, bidiag_layout, step):
    """The Householder reduction without the QR iteration: the 40-digit singular values of every 16x16 upper bidiagonal
    (d, e) the kernel leaves behind equal those of the integer matrix within 1e-13 sigma_max (every design under the
    default layout, every third under the other one)."""
    designs, _, _, quartets, _ = small
    pick = list(range(0, len(designs), step))
    q = quartets[pick]
    _configure(engine, 1, bidiag_layout)
    engine.set_option("svd_streams", 1)
    engine.set_option("svd_chunk", len(q))
    try:
        engine.resolve(q, False)
        de = engine.debug_fetch("de", len(q)).reshape(len(q), 3, 32)
    finally:
        engine.set_option("svd_streams", 0)
        engine.set_option("svd_chunk", 0)
        _configure(engine, 1, 1)
    assert np.isfinite(de).all() and (de[:, :, 16] == 0).all()
    worst, at = 0.0, None
    for n, i in enumerate(pick):
        svds, _, _ = D.mp_reference(D.flattenings(designs[i].m))
        for t in range(3):
            got = D.mp_bidiag_svd(de[n, t, :16], de[n, t, 16:])
            err = float(np.abs(got - svds[t]).max() / svds[t, 0])
            if err > worst:
                worst, at = err, (designs[i], t)
    print(f"[bidiagonalisation alone, {name}]: worst |sigma(B) - sigma_mp| / sigma_max = {worst:.3e} at {at} "
          f"({3 * len(pick)} matrices)")
    assert worst <= BIDIAG_BAR, f"{name}: {worst:.3e} sigma_max at {at}"


def _orders_batch(n_min=64):
    rows = [(0, p) for p in D.PERMS] * (-(-n_min // 24))
    return rows


@pytest.mark.parametrize("which", range(len(D.big_designs())))
def test_big_designs(which):
    """The designs with up to 2.1 M sites, each in a data set of its own (T = 4), scanned by the cooperative kernels:
    the 24 taxon orders, three times over, all SVD configurations, both modes."""
    from tetrad_amd.engine import QuartetEngine
    d = D.big_designs()[which]
    (tmparr, tmpmap, quartets), = D.realise([d], pack=False, seed=which)
    case = Case([d], quartets, _orders_batch())
    with QuartetEngine(0) as eng:
        eng.set_option("wg_min_quartets", 64)
        eng.set_option("dp_min_quartets", 2)
        eng.set_data(tmparr, tmpmap)
        for name, svd_method, bidiag_layout in SVD_CONFIGS:
            _configure(eng, svd_method, bidiag_layout)
            for sub in (True, False):
                case.judge(*eng.resolve(case.q, sub, debug=True), f"[{d.name}: {name}, sub={int(sub)}]")


# ---------------------------------------------------------------------------------------------------
# tq_bdsqr_kernel alone
# ---------------------------------------------------------------------------------------------------
def _de(d, e):
    return np.concatenate([d, e])


def _bdsqr_reference(cases):
    """40-digit singular values per case; the 2^32-scaled twins are the same values times 2^32 (exact in binary)."""
    half = len(cases) // 2
    ref = [D.mp_bidiag_svd(d, e) for _, _, d, e in cases[:half]]
    return np.stack(ref + [r * 2.0 ** 32 for r in ref])


def test_bdsqr_alone_on_bidiagonals_counts_cannot_reach():
    """`debug_bdsqr` on the designed bidiagonals: every value within 1e-12 sigma_max of the 40-digit one, none handed
    over with the not-converged sign, at most 60 sweeps per value; the cancel family really takes the cancel branch (its
    rotation-step counters differ from those of the same matrix with the diagonal zeros replaced by ones: the smaller of
    the two ways to show it, no counter added to the kernel); tile guards and lane positions (nmat 1, 2, 63, 64, 65,
    127, 129 with the cases rotated through the lanes) give bitwise what each matrix gives alone."""
    from tetrad_amd.engine import QuartetEngine
    cases = D.bidiagonal_cases()
    ref = _bdsqr_reference(cases)
    de = np.stack([_de(d, e) for _, _, d, e in cases])
    with QuartetEngine(0) as eng:
        sv, steps, sweeps, _ = eng.debug_bdsqr(de, reps=1)
        assert not np.signbit(sv).any(), "a value came back with the not-converged sign: " + \
            ", ".join(cases[i][0] for i in np.flatnonzero(np.signbit(sv).any(axis=1)))
        assert np.isfinite(sv).all()
        got = -np.sort(-sv, axis=1)
        smax = ref[:, :1]
        err = np.abs(got - ref) / np.where(smax > 0, smax, 1.0)
        for i in np.argsort(-err.max(axis=1))[:5]:
            print(f"[bdsqr alone] {cases[i][0]}: {err[i].max():.3e} sigma_max, {steps[i]} steps, {sweeps[i]} sweeps")
        print(f"[bdsqr alone] worst |sigma_dev - sigma_mp| / sigma_max = {err.max():.3e}; most sweeps {sweeps.max()}")
        assert (got[smax[:, 0] == 0] == 0).all(), "the zero matrix must give exact zeros"
        assert err.max() <= SIGMA_BAR, f"{cases[int(np.argmax(err.max(axis=1)))][0]}: {err.max():.3e} sigma_max"
        assert (sweeps <= 60 * 16).all(), f"sweeps {sweeps.max()}"       # 60 per value is the kernel's cap: the sign check above
        # cancel branch reached
        idx = [i for i, c in enumerate(cases) if c[1] == "cancel"]
        twin = de[idx].copy()
        dz = twin[:, :16] == 0
        for r in range(len(idx)):
            unit = 2.0 ** 32 if cases[idx[r]][0].endswith("x 2^32") else 1.0
            twin[r, :16][dz[r]] = unit
        _, steps_t, sweeps_t, _ = eng.debug_bdsqr(twin, reps=1)
        same = [(cases[i][0]) for r, i in enumerate(idx) if steps[i] == steps_t[r] and sweeps[i] == sweeps_t[r]]
        assert not same, f"no trace of the cancel branch in the work counters of {same}"
        # with the whole diagonal zero no sweep runs at all: the values can only come from the cancel branch's rotations
        for i in idx:
            if not cases[i][2].any():
                assert steps[i] == 0 and sweeps[i] == 0, cases[i][0]
        # tile guards and lane position
        alone = [eng.debug_bdsqr(de[i:i + 1], reps=1)[:3] for i in range(len(de))]
        for i, (s1, st1, sw1) in enumerate(alone):
            np.testing.assert_array_equal(s1[0], sv[i], err_msg=cases[i][0])
            assert st1[0] == steps[i] and sw1[0] == sweeps[i]
        hard = np.argsort(-steps.astype(np.int64), kind="stable")
        for nmat in (1, 2, 63, 64, 65, 127, 129):
            for rot in (0, 1, 17, 63):
                pick = hard[(np.arange(nmat) + rot) % len(hard)]
                s, st, sw, _ = eng.debug_bdsqr(de[pick], reps=1)
                np.testing.assert_array_equal(s, sv[pick], err_msg=f"nmat={nmat} rot={rot}")
                np.testing.assert_array_equal(st, steps[pick])
                np.testing.assert_array_equal(sw, sweeps[pick])


SCAN_DEFAULTS = {"park_t": 1, "scan_pair": 0, "share_c": 0, "scan_wg": 0, "scan_method": -1, "scan_dp": 1, "scan_f4": -1}


def _scan_options(sub):
    """The option list of test_gpu_configs.test_scan_kernel_variants_agree_on_sorted_batches."""
    return ({"park_t": 0}, {"scan_pair": 1}, {"scan_pair": 1, "scan_method": 1 - int(sub)}, {"share_c": 1},
            {"scan_wg": 8}, {"scan_method": 1 - int(sub)}, {"scan_method": 6}, {"scan_method": int(sub)},
            {"scan_dp": 0}, {"scan_f4": 1}, {"scan_f4": 0}, {"scan_f4": 0, "scan_dp": 0}, {"scan_wg": 8, "scan_f4": 0})


@pytest.mark.parametrize("S", [65_535, 65_536, 65_537, 1023 * 2048, 1023 * 2048 + 1])
@pytest.mark.parametrize("patterns", [((0, 1, 2, 3),), ((0, 1, 2, 3), (2, 0, 3, 1))], ids=["one-pattern", "two-patterns"])
def test_concentrated_patterns_at_the_counter_limits(S, patterns):
    """All S sites of four taxa carry one pattern (or two in turn): a single cell of the count matrix takes every
    increment.  Around 2^16 (the width of the bank-private counters of scan_pb.hpp) and at 1023 * 2048 sites, the
    largest S at which scan_method 6 still selects those counters (64 increments per step at most, 1023 steps), plus one
    site more, where it must fall back.  Every scan variant returns the design and, bit for bit, the default form's rows."""
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap, quartets, d = D.concentrated(S, patterns)
    case = Case([d], quartets, _orders_batch())
    with QuartetEngine(0) as eng:
        eng.set_option("wg_min_quartets", 64)
        eng.set_option("dp_min_quartets", 2)
        eng.set_data(tmparr, tmpmap)
        for sub in (True, False):
            base = eng.resolve(case.q, sub, debug=True)
            case.judge(*base, f"[S={S} x{len(patterns)}, sub={int(sub)}, default]")
            for opts in _scan_options(sub):
                for k, v in opts.items():
                    eng.set_option(k, v)
                try:
                    got = eng.resolve(case.q, sub, debug=True)
                finally:
                    for k in opts:
                        eng.set_option(k, SCAN_DEFAULTS[k])
                np.testing.assert_array_equal(got[3]["cmats"], case.cmats, err_msg=f"S={S} {opts} sub={sub}: cmats")
                for a, b in zip(base[:3], got[:3]):
                    np.testing.assert_array_equal(a, b, err_msg=f"S={S} {opts} sub={sub}")
                np.testing.assert_array_equal(base[3]["svds"], got[3]["svds"], err_msg=f"S={S} {opts} sub={sub}: svds")
