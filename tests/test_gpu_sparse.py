"""GPU: RAD-seq-like sparse inputs at benchmark shape (synth.RAD_PROFILES: whole loci missing per sample, a fifth
of the taxa 85-98 % missing, one dead taxon in rad85) against the oracle, judged by the exact bar of
tests/exact_ties.py: exact ranks decide which scores are exactly zero, so tied and near-tied rows -- 40 % of the
subsample rows of rad85 -- are checked too instead of being excused.

The oracle's rows (and the exact ranks of their count matrices) are computed once per module and shared by the
three engines of test_gpu_parity.py's ``engine`` fixture."""
import zlib
from functools import lru_cache

import numpy as np
import pytest

from conftest import load_golden
from exact_ties import check_rows, exact_rank, zero_tail_set
from test_gpu_parity import engine  # noqa: F401  (the three-engine fixture)

pytestmark = pytest.mark.gpu

PROFILES = ["rad30", "rad60", "rad85"]
SPARSE = 0.85          # taxa at least this much missing: the dead and the 85-98 % ones


@lru_cache(maxsize=None)
def profile_data(name):
    from tetrad_amd import synth
    return synth.radseq_profile(name)


def structured_quartets(tmparr, seed, n=2003):
    """~n quartets in (a,b,c)-sorted order: runs of equal (a,b,c) of length 1-7 (a few of 9-17, beyond the
    joint-histogram pairing's short backward walk), d drawn from the sparse taxa as often as from the others,
    repeated quartets, (a,b) runs of every length so that aligned groups of four share (a,b) with their first
    quartet 1, 2, 3 or 4 times; n odd."""
    rng = np.random.default_rng(seed)
    T = tmparr.shape[0]
    miss = (tmparr == 78).mean(axis=1)
    sparse = set(np.flatnonzero(miss >= SPARSE).tolist())
    out = []
    while len(out) < n + 64:
        a = int(rng.integers(0, T // 2))
        b = int(rng.integers(a + 1, a + 1 + T // 4))
        for c in sorted(rng.choice(np.arange(b + 1, T - 8), size=int(rng.integers(1, 4)), replace=False).tolist()):
            above = np.arange(c + 1, T)
            pools = [p for p in (above[np.isin(above, list(sparse))], above[~np.isin(above, list(sparse))]) if len(p)]
            L = int(rng.integers(9, 18)) if rng.random() < 0.04 else int(rng.integers(1, 8))
            for _ in range(L):
                pool = pools[int(rng.integers(len(pools)))]
                q = (a, b, c, int(rng.choice(pool)))
                out.append(q)
                if rng.random() < 0.08:
                    out.append(q)                       # a repeated quartet
    q = np.array(out, np.uint32)
    q = q[np.lexsort((q[:, 3], q[:, 2], q[:, 1], q[:, 0]))]
    return np.ascontiguousarray(q[:n])


def paired_share(q):
    """Share of quartets that the joint-histogram scan pairs: runs of equal (a,b,c) in sorted order, two by two."""
    key = (q[:, 0].astype(np.int64) * 1024 + q[:, 1]) * 1024 + q[:, 2]
    key = np.sort(key)
    _, runs = np.unique(key, return_counts=True)
    return float((2 * (runs // 2)).sum() / len(q))


@lru_cache(maxsize=None)
def quartet_set(name, kind):
    from tetrad_amd import synth
    if kind == "random":
        return synth.random_quartets(128, 3000, seed=2024)
    return structured_quartets(profile_data(name)[0], seed=7)


def _oracle(tmparr, tmpmap, q, sub):
    from oracle import oracle as orc
    _, o_rstat, o_rscor, o = orc.new_infer_resolved_quartets(tmparr, tmpmap, q, sub, debug=True)
    live = o_rstat[:, 1] > 0
    exact = np.zeros((len(q), 3), np.int32)
    exact[live] = exact_rank(o["cmats"][live])
    return (o_rstat, o_rscor, o), exact


@lru_cache(maxsize=None)
def oracle_rows(name, kind, sub):
    tmparr, tmpmap = profile_data(name)
    return _oracle(tmparr, tmpmap, quartet_set(name, kind), sub)


def tie_counts(orc, exact):
    """Oracle-side counts: zero-data rows, exact ties (|Z| >= 2), lone zero scores (|Z| == 1), min rank < 10."""
    live = orc[0][:, 1] > 0
    z = np.array([len(zero_tail_set(r)) for r in exact[live]])
    return dict(rows=len(live), zero=int((~live).sum()), tie=int((z >= 2).sum()), one=int((z == 1).sum()),
                lowrank=int((exact[live].min(axis=1) < 10).sum()))


def resolve_twice(engine, q, sub):
    """Debug call (count matrices, singular values, ranks) and plain call: bitwise the same rows."""
    rstat, rscor, flags, dbg = engine.resolve(q, sub, debug=True)
    plain = engine.resolve(q, sub)
    for a, b, what in zip((rstat, rscor, flags), plain, ("rstat", "rscor", "flags")):
        np.testing.assert_array_equal(a, b, err_msg=f"debug vs plain call: {what}")
    return (rstat, rscor, flags), dbg


@pytest.mark.parametrize("profile", PROFILES)
def test_profiles_exercise_the_exact_bar(profile):
    """What the profiles are for, counted on the oracle side: rad85 has many exact ties and zero-data rows, rad60 many
    low-rank rows, and the structured set is mostly (a,b,c) pairs of the joint-histogram scan."""
    rand = {sub: tie_counts(*oracle_rows(profile, "random", sub)) for sub in (True, False)}
    struct = {sub: tie_counts(*oracle_rows(profile, "structured", sub)) for sub in (True, False)}
    print(profile, "random", rand, "structured", struct)
    if profile == "rad85":
        assert rand[True]["tie"] >= 0.20 * rand[True]["rows"], rand
        assert rand[True]["zero"] >= 0.01 * rand[True]["rows"], rand
    if profile == "rad60":
        for sub in (True, False):
            assert rand[sub]["lowrank"] >= 0.05 * rand[sub]["rows"], rand
    q = quartet_set(profile, "structured")
    assert len(q) % 4 and paired_share(q) >= 0.8
    ab = q[:, 0].astype(np.int64) * 1024 + q[:, 1]
    g = ab[: len(q) // 4 * 4].reshape(-1, 4)
    assert {1, 2, 3, 4} <= set((g == g[:, :1]).sum(axis=1).tolist())
    assert (q[1:] == q[:-1]).all(axis=1).any()              # repeated quartets
    miss = (profile_data(profile)[0] == 78).mean(axis=1)
    assert 0.3 <= float(np.mean(miss[q[:, 3]] >= SPARSE)) <= 0.7


@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("profile", PROFILES)
def test_sparse_profile_vs_oracle_exact_bar(engine, profile, kind):
    """3 000 random / ~2 000 structured quartets of a c3-shaped sparse input, both modes: count matrices, nsnps and
    ranks exact, values to tolerance, ties and near-ties judged exactly; the plain call == the debug call."""
    tmparr, tmpmap = profile_data(profile)
    q = quartet_set(profile, kind)
    engine.set_data(tmparr, tmpmap)
    for sub in (True, False):
        dev, dbg = resolve_twice(engine, q, sub)
        orc, exact = oracle_rows(profile, kind, sub)
        n = check_rows(dev, dbg, orc, exact)
        print(profile, kind, "sub" if sub else "full", n)


def test_sorted_batch_default_options():
    """40 000 rad85 quartets (above the device-sort / joint-histogram threshold) under the default options == the
    same quartets as 3 000-quartet unsorted chunks, debug call == plain call, and the exact bar on 3 000 rows."""
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap = profile_data("rad85")
    first = quartet_set("rad85", "random")
    q = np.concatenate([first, synth.random_quartets(128, 40_000 - len(first), seed=99)])
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        for sub in (True, False):
            dev, dbg = resolve_twice(eng, q, sub)
            chunks = [eng.resolve(q[i:i + 3000], sub) for i in range(0, len(q), 3000)]
            for k, what in enumerate(("rstat", "rscor", "flags")):
                np.testing.assert_array_equal(dev[k], np.concatenate([c[k] for c in chunks]), err_msg=f"sorted vs chunks: {what}")
            orc, exact = oracle_rows("rad85", "random", sub)
            n = len(first)
            check_rows(tuple(x[:n] for x in dev), {k: v[:n] for k, v in dbg.items()}, orc, exact)


def test_sparse_c4_shape_default_options():
    """1 000 rad60 quartets at the c4 shape (256 taxa, 100 000 sites) under the default options."""
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    T, S, _ = synth.CONFIGS["c4"]
    tmparr, tmpmap = synth.radseq_profile("rad60", T=T, S=S, seed=synth.CONFIG_SEEDS["c4"])
    q = synth.random_quartets(T, 1000, seed=404)
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        for sub in (True, False):
            dev, dbg = resolve_twice(eng, q, sub)
            orc, exact = _oracle(tmparr, tmpmap, q, sub)
            print("c4 rad60", "sub" if sub else "full", check_rows(dev, dbg, orc, exact))


_c5_oracle = {}


def test_sparse_c5_device_replicate_vs_oracle(engine):
    """A bootstrap source made from rad60 (N for missing, IUPAC codes), one replicate built on the device and exported,
    1 500 quartets on it against the oracle under the exact bar (no "no flags" shortcut)."""
    from tetrad_amd import bootstrap, synth
    seqarr, maparr, spans = synth.make_c5_source(source=profile_data("rad60"))
    engine.set_source(seqarr, spans)
    rng = np.random.default_rng(synth.CONFIG_SEEDS["c5"])
    lidxs, s1, s2 = bootstrap.draw_replicate(len(spans), rng)
    S = engine.bootstrap(lidxs, s1, s2)
    tmparr, tmpmap = engine.get_data()
    assert tmparr.shape == (128, S) and (tmparr == 78).mean() > 0.5
    q = synth.random_quartets(128, 1500, seed=56)
    key = zlib.crc32(tmparr.tobytes())
    for sub in (True, False):
        dev, dbg = resolve_twice(engine, q, sub)
        if (key, sub) not in _c5_oracle:                    # the replicate is the same under every engine
            _c5_oracle[key, sub] = _oracle(tmparr, tmpmap, q, sub)
        orc, exact = _c5_oracle[key, sub]
        print("c5 rad60", "sub" if sub else "full", check_rows(dev, dbg, orc, exact))


def test_reference_sparse_slice(engine):
    """tests/golden/sparse_c3_slice.npz: the reference's own rows, count matrices and singular values for 96 quartets
    each of rad60 and rad85 at c3 shape (regenerated input, CRC-checked); the device under the exact bar."""
    from tetrad_amd import synth
    g = load_golden("sparse_c3_slice")
    for profile in ("rad60", "rad85"):
        tmparr, tmpmap = profile_data(profile)
        assert zlib.crc32(tmparr.tobytes()) == int(g[f"{profile}_tmparr_crc32"])
        assert zlib.crc32(np.ascontiguousarray(tmpmap).tobytes()) == int(g[f"{profile}_tmpmap_crc32"])
        engine.set_data(tmparr, tmpmap)
        q = g[f"{profile}_quartets"]
        for mode in ("full", "sub"):
            dev, dbg = resolve_twice(engine, q, mode == "sub")
            sv = g[f"{profile}_{mode}_svds"]
            ref = dict(cmats=g[f"{profile}_{mode}_cmats"], svds=sv,
                       rank=(sv > sv.max(axis=2, keepdims=True) * 16 * np.finfo(float).eps).sum(axis=2))
            check_rows(dev, dbg, (g[f"{profile}_{mode}_rstat"], g[f"{profile}_{mode}_rscor"], ref))
    assert synth.RAD_PROFILES["rad85"]["dead_taxa"] == 1
