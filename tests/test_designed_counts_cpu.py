"""CPU: the designed count matrices of tests/designed_counts.py and their 40-digit reference, pinned so that the GPU
test (tests/test_gpu_designed_svd.py) cannot pass for the wrong reason: the realised data give exactly the designs,
the designs are what their families claim, no design needs to be excluded from a rank comparison, and LAPACK in f64
meets -- a hundred times over -- the bar the device is held to."""
import collections

import numpy as np
import pytest

import designed_counts as D
import exact_ties as X

DEVICE_BAR = 1e-12          # |sigma_dev - sigma_mp| <= DEVICE_BAR * sigma_max in the GPU test
LAPACK_BAR = 1e-14


@pytest.fixture(scope="module")
def designs():
    return D.small_designs() + D.large_designs()


@pytest.fixture(scope="module")
def refs(designs):
    """(cmats [N,3,16,16], [(svds, ranks, scores)]) of every design; the 40-digit values are cached for the session."""
    cm = np.stack([D.flattenings(d.m) for d in designs])
    return cm, [D.mp_reference(c) for c in cm]


def test_realise_rejects_invariant_cells_and_bad_shapes():
    m = np.zeros((16, 16), np.int64)
    m[1, 2] = 3
    D.realise([m])
    for k in D.INVARIANT:
        bad = m.copy()
        bad[k, k] = 1
        with pytest.raises(ValueError):
            D.realise([m, bad])
    with pytest.raises(ValueError):
        D.realise([np.zeros((4, 4), np.int64)])


def test_realisation_is_exact_in_both_modes(oracle):
    """The oracle's count matrices of the realised data are the designs (and their two other flattenings), in subsample
    mode and in full mode, for the packed data set of all small designs, shuffled sites or not."""
    small = D.small_designs()
    want = np.stack([D.flattenings(d.m) for d in small])
    assert 250 <= len(small) <= 350
    for seed in (None, 3):
        tmparr, tmpmap, quartets = D.realise(small, seed=seed)
        assert tmparr.shape == (4 * len(small), sum(d.sites for d in small)) and len(quartets) == len(small)
        assert len(np.unique(tmpmap[:, 0])) == tmparr.shape[1], "every site must be its own locus"
        # a design's taxa are missing at every other design's sites
        live = (tmparr != D.MISSING).reshape(len(small), 4, -1)
        assert (live.all(axis=1) == live.any(axis=1)).all() and (live.any(axis=1).sum(axis=0) == 1).all()
        for sub in (True, False):
            _, rstat, _, dbg = oracle.new_infer_resolved_quartets(tmparr, tmpmap, quartets, sub, debug=True)
            np.testing.assert_array_equal(dbg["cmats"], want, err_msg=f"sub={sub} seed={seed}")
            np.testing.assert_array_equal(rstat[:, 1], [d.sites for d in small])


def test_realisation_under_all_taxon_orders(oracle):
    """All 24 orders of a quartet's four taxa: the oracle's matrices on the realised data are `flattenings(m, order)`,
    the pure-Python count loop agrees on a few, and the flattening map used for the reordered references
    (`flattening_of_order`) holds for the singular values and the exact ranks."""
    small = D.small_designs()
    pick = [i for i, d in enumerate(small) if d.name.endswith("seed=0") or d.family == "a"][::3]
    assert len(pick) >= 12 and len({small[i].family for i in pick}) >= 5
    tmparr, tmpmap, quartets = D.realise(small, seed=5)
    q = np.stack([quartets[i][list(p)] for i in pick for p in D.PERMS])
    want = np.stack([D.flattenings(small[i].m, p) for i in pick for p in D.PERMS])
    for sub in (True, False):
        _, _, _, dbg = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q, sub, debug=True)
        np.testing.assert_array_equal(dbg["cmats"], want)
    for j in (0, 7, 23, 24 * 3 + 11, len(q) - 1):
        seqs = tmparr[q[j]]
        mask = (seqs >= 78).any(axis=0) | (seqs == seqs[0]).all(axis=0)
        keep = ~mask                                     # the interpreted loop is slow: hand it the counted sites only
        for sub in (True, False):
            got = oracle.chunk_to_matrices_py(seqs[:, keep], tmpmap[keep, 0], mask[keep], sub)
            np.testing.assert_array_equal(got, want[j])
    exact = X.exact_rank(want)
    sv = np.linalg.svd(want.astype(np.float64), compute_uv=False)
    for n, i in enumerate(pick):
        ref = D.mp_reference(D.flattenings(small[i].m))
        for k, p in enumerate(D.PERMS):
            svds, ranks, _ = D.reorder_reference(ref, p)
            np.testing.assert_array_equal(exact[24 * n + k], ranks)
            assert np.abs(sv[24 * n + k] - svds).max() <= LAPACK_BAR * svds.max()


def test_concentrated_data_sets(oracle):
    """One pattern at every site, and two patterns in turn: the single cells hold S, or S split in two."""
    for S in (1, 2, 65_537):
        for pats in (((0, 1, 2, 3),), ((0, 1, 2, 3), (3, 3, 0, 1))):
            tmparr, tmpmap, q, d = D.concentrated(S, pats)
            assert d.sites == S and (d.m > 0).sum() == min(len(pats), S)
            for sub in (True, False):
                _, rstat, _, dbg = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q, sub, debug=True)
                np.testing.assert_array_equal(dbg["cmats"][0], D.flattenings(d.m))


def test_large_designs_realise_exactly(oracle):
    for d in D.big_designs():
        (tmparr, tmpmap, q), = D.realise([d], pack=False)
        assert tmparr.shape == (4, d.sites)
        for sub in (True, False):
            _, _, _, dbg = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q, sub, debug=True)
            np.testing.assert_array_equal(dbg["cmats"][0], D.flattenings(d.m))
    assert max(d.sites for d in D.big_designs()) > 1023 * 2048, "the graded designs also pass the bank-private limit"


def test_designs_are_what_they_claim(designs, refs):
    cm, ref = refs
    names = [d.name for d in designs]
    assert len(set(names)) == len(names)
    fam = collections.Counter(d.family for d in designs)
    assert set(fam) == {"a", "b", "c", "c+", "d", "e", "f"}
    ranks = np.stack([r[1] for r in ref])
    for d, r in zip(designs, ranks):
        if d.rank is not None:
            assert r[0] == d.rank, f"{d}: exact rank {r[0]}, designed {d.rank}"
    assert {d.rank for d in designs if d.family == "b"} == set(range(1, 17))
    assert {d.rank for d in designs if d.family == "a"} == set(range(1, 17))
    # the min(10, ...) cap of the score rule is pinned from both sides, and the full-rank case is there
    minrank = collections.Counter(ranks.min(axis=1).tolist())
    for r in (8, 9, 10, 11, 12, 16):
        assert minrank[r] >= 5, f"only {minrank[r]} quartets whose smallest exact rank is {r}"
    # (a) and (c) really have repeated singular values in the 40-digit SVD: equal to 1e-30 relative
    for d, (svds, rk, _) in zip(designs, ref):
        s = svds[0][:rk[0]]
        if d.family == "a":
            assert len(s) == d.equal and np.abs(s - s[0]).max() <= 1e-30 * s[0], d
        if d.family == "c":
            groups = s.reshape(-1, d.equal)
            assert np.abs(groups - groups[:, :1]).max() <= 1e-30 * s[0], d
            assert len(np.unique(groups[:, 0])) >= 2, d
    # the exact-tie rule and the lone-zero rule of check_topology both have designs to judge
    z = collections.Counter(len(X.zero_tail_set(r)) for r in ranks)
    assert z[0] >= 20 and z[1] >= 20 and z[2] + z[3] >= 20, z


def test_no_design_needs_excluding_from_the_rank_comparison(designs, refs):
    """The smallest non-zero 40-digit singular value of every flattening is at least 1e-9 sigma_max: five decades above
    the rank threshold 16 eps sigma_max = 3.6e-15 sigma_max, and the values below the exact rank are exactly zero, so a
    device within 1e-12 sigma_max of the reference must report the exact rank of every matrix."""
    _, ref = refs
    worst = 1.0
    for d, (svds, rk, _) in zip(designs, ref):
        for t in range(3):
            if rk[t]:
                ratio = svds[t, rk[t] - 1] / svds[t, 0]
                worst = min(worst, ratio)
                assert ratio >= 1e-9, f"{d} flattening {t}: smallest non-zero singular value {ratio:.2e} sigma_max"
    print(f"smallest non-zero singular value over all designs: {worst:.2e} sigma_max")
    assert worst > 1e3 * DEVICE_BAR


def test_lapack_meets_the_device_bar_a_hundred_times_over(designs, refs):
    """|sigma_numpy - sigma_mp| <= 1e-14 sigma_max on every design, and numpy's rank rule gives the exact ranks: the
    device bar of 1e-12 sigma_max asks for nothing an f64 algorithm of this class cannot do."""
    cm, ref = refs
    sv = np.linalg.svd(cm.astype(np.float64), compute_uv=False)
    worst = 0.0
    for i, (d, (svds, rk, _)) in enumerate(zip(designs, ref)):
        err = np.abs(sv[i] - svds).max() / svds.max()
        worst = max(worst, err)
        assert err <= LAPACK_BAR, f"{d}: numpy is {err:.2e} sigma_max away from the 40-digit values"
        np.testing.assert_array_equal((sv[i] > sv[i, :, :1] * 16 * np.finfo(np.float64).eps).sum(axis=1), rk)
    print(f"worst |sigma_numpy - sigma_mp| / sigma_max over {len(designs)} designs: {worst:.2e}")
    assert 100 * LAPACK_BAR <= DEVICE_BAR


def test_mp_scores_agree_with_the_adjudicator_and_the_oracle(designs, refs, oracle):
    """`mp_reference` scores == `exact_ties.mp_scores` with the exact minrank (two routes to the same 40 digits, one with
    the exact zeros put in), and the oracle's f64 scores are within the project bar of them."""
    cm, ref = refs
    for i in range(0, len(designs), 7):
        svds, rk, scores = ref[i]
        other = X.mp_scores(cm[i], min(10, int(rk.min())))
        assert np.abs(other - scores).max() <= 1e-15 * svds.max(), designs[i]      # the f64 rounding of the values
        _, _, o_scores, _ = oracle.score_from_cmats(cm[i])
        assert (np.abs(o_scores - scores) <= 1e-6 * np.abs(scores) + 1e-12 * svds.max()).all(), designs[i]


def test_bidiagonal_cases_cover_what_the_issue_lists():
    cases = D.bidiagonal_cases()
    kinds = collections.Counter(k for _, k, _, _ in cases)
    assert kinds["cancel"] >= 20 and kinds["split"] >= 2 * (15 + 8)
    names = [n for n, *_ in cases]
    assert len(set(names)) == len(names) and len(cases) % 2 == 0
    half = len(cases) // 2
    for (n, k, d, e), (n2, k2, d2, e2) in zip(cases[:half], cases[half:]):
        assert e[0] == 0 and k == k2
        np.testing.assert_array_equal(d * 2.0 ** 32, d2)
        np.testing.assert_array_equal(e * 2.0 ** 32, e2)
        if k == "cancel":                      # an exact zero on the diagonal with a live superdiagonal to its right
            assert any(d[i] == 0 and e[i + 1] != 0 for i in range(15)), n
    # the 40-digit reference of a bidiagonal against values known in closed form
    np.testing.assert_allclose(D.mp_bidiag_svd(np.arange(1.0, 17), np.zeros(16)), np.arange(16.0, 0, -1), rtol=1e-15)
    e = np.arange(16.0)
    np.testing.assert_allclose(D.mp_bidiag_svd(np.zeros(16), e), np.arange(15.0, -1, -1), rtol=1e-15, atol=1e-30)
    # Toeplitz d = e = 1: sigma_j = 2 cos(j pi / 33), j = 1..16
    want = 2 * np.cos(np.arange(1, 17) * np.pi / 33)
    np.testing.assert_allclose(D.mp_bidiag_svd(np.ones(16), np.ones(16)), want, rtol=1e-14)
