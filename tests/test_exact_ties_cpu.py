"""CPU: the exact adjudicator of tests/exact_ties.py and the RAD-seq-like generator synth.simulate_radseq."""
import zlib

import numpy as np
import pytest

import exact_ties as X


def _rank_cases():
    rng = np.random.default_rng(0)
    for _ in range(150):                                                    # random integer matrices, mostly full rank
        yield rng.integers(0, rng.choice([2, 5, 1000, 60_000]), size=(16, 16))
    for r in range(17):                                                     # products of rank r
        for _ in range(6):
            yield rng.integers(0, 6, size=(16, r)) @ rng.integers(0, 6, size=(r, 16))
    for _ in range(60):
        m = rng.integers(0, 9, size=(16, 16))
        kind = rng.integers(4)
        if kind == 0:                                                       # repeated rows
            m[rng.integers(0, 16, 6)] = m[rng.integers(0, 16)]
        elif kind == 1:                                                     # repeated columns
            m[:, rng.integers(0, 16, 9)] = m[:, [rng.integers(0, 16)]]
        elif kind == 2:                                                     # zero blocks
            i, j = rng.integers(1, 16, 2)
            m[:i, :j] = 0
            m[i:, j:] = 0
        else:                                                               # count-matrix-like: sparse, a few live rows
            m[rng.random(m.shape) < 0.85] = 0
        yield m
    yield np.zeros((16, 16), np.int64)


def test_exact_rank_equals_numpy_rank():
    cases = list(_rank_cases())
    got = X.exact_rank(np.stack(cases).astype(np.uint32))
    want = [np.linalg.matrix_rank(m.astype(np.float64)) for m in cases]
    np.testing.assert_array_equal(got, want)
    assert set(range(17)) <= set(got.tolist())
    # the modular lower bound never exceeds the rank, and Bareiss alone gives the same ranks
    assert (X._rank_mod_p(np.stack(cases)) <= got).all()
    np.testing.assert_array_equal([X._rank_one(m) for m in cases], want)


def test_exact_rank_where_floating_point_cannot_tell():
    """A nearly singular integer matrix: exact rank 16 (det = 1) although its smallest singular value is tiny, and a
    singular one with huge entries."""
    n = 16
    m = np.eye(n, dtype=object)
    for i in range(n - 1):
        m[i, i + 1] = 60                                                    # unit upper bidiagonal: det 1, sigma_min ~ 60^-15
    assert X._rank_one(np.array(m, dtype=np.int64)) == 16
    big = np.random.default_rng(1).integers(0, 50_000, size=(16, 15)).astype(np.int64)
    big = np.concatenate([big, big[:, :1] * 3 - big[:, 1:2]], axis=1)       # column 15 = 3 col0 - col1
    assert X._rank_one(big) == 15


@pytest.mark.parametrize("ranks,Z", [
    ((4, 4, 7), {0, 1}), ((4, 5, 7), {0}), ((3, 3, 3), {0, 1, 2}), ((10, 11, 12), {0}), ((10, 10, 16), {0, 1}),
    ((11, 12, 16), set()), ((16, 16, 16), set()), ((0, 2, 0), {0, 2}), ((9, 16, 12), {0}), ((12, 9, 9), {1, 2}),
])
def test_zero_tail_set(ranks, Z):
    assert X.zero_tail_set(ranks) == Z


def test_mp_scores_exact_zeros_and_values():
    rng = np.random.default_rng(3)
    low = rng.integers(0, 6, size=(16, 3)) @ rng.integers(0, 6, size=(3, 16))
    full = rng.integers(0, 6, size=(16, 16))
    cm = np.stack([low, low.T, full]).astype(np.uint32)
    sc = X.mp_scores(cm, 3)
    sv = np.linalg.svd(full.astype(np.float64), compute_uv=False)
    assert sc[0] <= 1e-30 * sv[0] and sc[1] <= 1e-30 * sv[0] and sc[2] > 1e-3 * sv[0]
    assert abs(sc[2] - np.sqrt((sv[3:] ** 2).sum())) <= 1e-12 * sv[0]


@pytest.fixture(scope="module")
def sparse_rows(oracle):
    """The oracle's rows on a small sparse RAD-like input, with its exact ranks."""
    from tetrad_amd import synth
    tmparr, tmpmap = synth.simulate_radseq(14, 1500, seed=5, block=0.7, cell=0.02, hi_frac=0.2, dead_taxa=1)
    q = synth.all_quartets(14)
    _, r, s, o = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q, True, debug=True)
    return r, s, o


def _as_device(rows):
    r, s, o = rows
    return [r.copy(), s.copy(), o["flags"].copy()], dict(cmats=o["cmats"], svds=o["svds"], ranks=o["rank"])


def test_check_rows_accepts_the_oracle_and_counts_every_kind(sparse_rows):
    dev, dbg = _as_device(sparse_rows)
    n = X.check_rows(tuple(dev), dbg, sparse_rows)
    assert n["zero"] > 0 and n["tie"] > 0 and n["one"] > 0 and n["lowrank"] > 0
    assert n["rows"] == n["zero"] + n["tie"] + n["one"] + n["empty"]


def _first(rows, want):
    """First row with |Z| of the wanted kind (exact ranks of the oracle's count matrices)."""
    r, _, o = rows
    for i in np.flatnonzero(r[:, 1] > 0):
        if want(len(X.zero_tail_set(X.exact_rank(o["cmats"][i])))):
            return i
    raise AssertionError("no such row")


@pytest.mark.parametrize("wrong", ["tie_topology", "tie_unflagged", "lone_zero_topology", "lone_zero_overeager_flag",
                                   "rank", "zero_data_flag", "cmats", "sweep_cap"])
def test_check_rows_rejects(sparse_rows, wrong):
    """Each kind of wrong device row makes the bar fail."""
    (rstat, rscor, flags), dbg = _as_device(sparse_rows)
    dbg = {k: v.copy() for k, v in dbg.items()}
    if wrong.startswith("tie"):
        i = _first(sparse_rows, lambda z: z == 2)
        Z = X.zero_tail_set(X.exact_rank(dbg["cmats"][i]))
        if wrong == "tie_topology":
            rstat[i, 0] = ({0, 1, 2} - Z).pop()
        else:
            flags[i] &= ~np.uint8(2)
    elif wrong.startswith("lone_zero"):
        i = _first(sparse_rows, lambda z: z == 1)
        (z,) = X.zero_tail_set(X.exact_rank(dbg["cmats"][i]))
        if wrong == "lone_zero_topology":
            rstat[i, 0] = (z + 1) % 3
        else:
            flags[i] |= 2
    elif wrong == "rank":
        i = _first(sparse_rows, lambda z: z >= 1)
        dbg["ranks"][i, 0] += 1
    elif wrong == "zero_data_flag":
        flags[int(np.flatnonzero(rstat[:, 1] > 0)[0])] |= 1
    elif wrong == "cmats":
        dbg["cmats"][3, 1, 2, 3] += 1
    else:
        flags[5] |= 8
    with pytest.raises(AssertionError):
        X.check_rows((rstat, rscor, flags), dbg, sparse_rows)


@pytest.mark.parametrize("name", ["rad30", "rad60", "rad85"])
def test_radseq_profiles_hit_their_missing_share(name):
    from tetrad_amd import synth
    tmparr, tmpmap = synth.radseq_profile(name)
    assert tmparr.shape == (128, 50_000) and tmpmap.shape == (50_000, 2)
    assert abs((tmparr == 78).mean() - synth.RAD_PROFILES[name]["target"]) <= 0.02
    loc = tmpmap[:, 0].astype(np.int64)
    assert (np.diff(loc) >= 0).all() and (np.diff(np.unique(loc)) > 1).any()          # non-decreasing, with gaps
    miss = (tmparr == 78).mean(axis=1)
    assert (miss >= 0.85).sum() >= 0.2 * 128 - 1
    assert (miss == 1.0).sum() == synth.RAD_PROFILES[name]["dead_taxa"]


def test_radseq_is_deterministic_and_missing_comes_in_loci():
    from tetrad_amd import synth
    kw = dict(block=0.5, cell=0.0, hi_frac=0.25, hi_range=(0.9, 0.95), dead_taxa=2)
    a1, m1 = synth.simulate_radseq(20, 3000, 17, **kw)
    a2, m2 = synth.simulate_radseq(20, 3000, 17, **kw)
    assert zlib.crc32(a1.tobytes()) == zlib.crc32(a2.tobytes()) and zlib.crc32(m1.tobytes()) == zlib.crc32(m2.tobytes())
    a3, _ = synth.simulate_radseq(20, 3000, 18, **kw)
    assert not np.array_equal(a1, a3)
    # with no cell-level missing, every locus of every taxon is either complete or entirely missing
    loc = m1[:, 0]
    for t in range(20):
        for ids in np.split(a1[t] == 78, np.flatnonzero(np.diff(loc)) + 1):
            assert ids.all() or not ids.any()
    # the same sites as simulate_tmparr without missing cells
    b, _ = synth.simulate_tmparr(20, 3000, 17, missing=0.0)
    live = a1 != 78
    np.testing.assert_array_equal(a1[live], b[live])


def test_radseq_profile_crc32_pins():
    """The sparse fixture (tests/golden/sparse_c3_slice.npz) regenerates its inputs from these profiles."""
    from conftest import load_golden
    from tetrad_amd import synth
    g = load_golden("sparse_c3_slice")
    for name in ("rad60", "rad85"):
        tmparr, tmpmap = synth.radseq_profile(name)
        assert zlib.crc32(tmparr.tobytes()) == int(g[f"{name}_tmparr_crc32"])
        assert zlib.crc32(np.ascontiguousarray(tmpmap).tobytes()) == int(g[f"{name}_tmpmap_crc32"])
