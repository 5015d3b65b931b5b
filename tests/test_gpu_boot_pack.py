"""GPU: option ``boot_pack`` -- the packed layout set of a device-built bootstrap replicate (csrc/bootstrap.hpp:
tq_boot_pack_map_kernel, tq_boot_pack_build_kernel; planned on the host at locus level, csrc/pack.hpp: PackPlanner).

A replicate built with ``boot_pack=1`` must resolve BITWISE like the same replicate (same draws, same seeds) built with
``boot_pack=0``: the count matrix is a histogram over loci, the layout only changes which lane counts which locus.

1. bitwise against the natural layout and against the oracle, every scan kernel, replicate lengths on and next to the
   2048-site step and the 32-site word;
2. the device's site map is the host packer's (tq_pack_sites on the exported tmpmap), entry for entry;
3. a packed set two steps longer than the natural one (beyond the 1/8 head-room of the natural buffers);
4. the life cycle of the packed buffers on one engine;
5. the readers of the natural set (full mode, species mode, tq_get_data) after a packed replicate;
6. replicates in flight (ReplicateRunner, both samplers);
7. the automatic rule (``boot_pack=-1``), decided once on the source.

Every test fails without the option."""
import numpy as np
import pytest

from test_gpu_bootstrap_layout import DEAD, L, LENGTHS, TILE, draws, layout_source, padded, quartet_sets
from test_gpu_site_packing import VARIANTS, resolve_all

pytestmark = pytest.mark.gpu

CODE = np.full(256, 78, np.uint8)
CODE[[65, 67, 71, 84]] = [0, 1, 2, 3]
CODE[[82, 75, 83, 89, 87, 77]] = [0, 3, 1, 1, 0, 0]          # a two-base IUPAC code counts as present (its first base)


def assert_same_rows(a, b, what):
    assert len(a) == len(b)
    for (name, x), (_, y) in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{what}: boot_pack 0 vs 1, {name}")


def rows_of(eng, qsets, variants=VARIANTS):
    return [r for q in qsets for r in resolve_all(eng, q, variants)]


def ascii_source(T, widths, seed):
    """(seqarr, spans) with loci of the given widths: ~15 % N, ~3 % IUPAC two-base codes."""
    from tetrad_amd import synth
    rng = np.random.default_rng(seed)
    widths = np.asarray(widths)
    ends = np.cumsum(widths)
    spans = np.stack([ends - widths, ends], axis=1).astype(np.int64)
    tmparr, _ = synth.simulate_tmparr(T, int(ends[-1]), seed=seed, missing=0.15)
    seqarr = np.where(tmparr <= 3, np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)], 78).astype(np.uint8)
    amb = rng.random(seqarr.shape) < 0.03
    seqarr[amb] = rng.choice(np.frombuffer(b"RKSYWM", np.uint8), size=int(amb.sum()))
    return seqarr, spans


@pytest.fixture(scope="module")
def source10():
    """Loci of 1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 2047, 2048 and 2100 sites + 60 of 1 + Poisson(3); ~15 % N, ~3 % IUPAC,
    one taxon all N, the first sites of the wide loci missing."""
    src = layout_source(10, seed=12)
    assert len(src[1]) == 73 and (src[0][DEAD] == 78).all()
    return src


@pytest.fixture(scope="module")
def pair():
    """(engine with boot_pack 0, engine with boot_pack 1)."""
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as E0, QuartetEngine(0) as E1:
        assert E0.set_option("boot_pack", 0) == 0
        E1.set_option("boot_pack", 1)
        yield E0, E1


def build_both(E0, E1, src, lidxs, seeds):
    S = None
    for E in (E0, E1):
        E.set_source(*src)
        got = E.bootstrap(lidxs, *seeds)
        assert S in (None, got)
        S = got
    assert E0.site_pack_state()[1] is False and E1.site_pack_state()[1] is True
    assert E1.site_pack_state()[0] >= padded(S) and E1.site_pack_state()[0] % TILE == 0
    return S


def test_option_values():
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        for v in (-1, 0, 1):
            eng.set_option("boot_pack", v)
        for v in (-2, 2):
            with pytest.raises(TetradHipError):
                eng.set_option("boot_pack", v)
        with pytest.raises(TetradHipError):
            eng.boot_pack_map()                                   # no replicate at all


# -- 1, 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LENGTHS))
def test_bitwise_against_the_natural_layout_and_the_oracle(pair, source10, oracle, name):
    from tetrad_amd.engine import pack_sites
    E0, E1 = pair
    first, S = LENGTHS[name]
    lidxs = draws(source10[1], first, S)
    assert build_both(E0, E1, source10, lidxs, (41, 43)) == S
    d0, d1 = E0.get_data(), E1.get_data()
    np.testing.assert_array_equal(d0[0], d1[0])
    np.testing.assert_array_equal(d0[1], d1[1])
    qsets = quartet_sets(10)
    assert len(qsets[0]) == 210
    r0, r1 = rows_of(E0, qsets), rows_of(E1, qsets)
    assert_same_rows(r0, r1, name)
    # the packed engine against the oracle on the exported replicate, both modes
    for sub in (True, False):
        rstat, _, _, dbg = E1.resolve(qsets[0], sub, debug=True)
        _, o_rstat, _, o = oracle.new_infer_resolved_quartets(d1[0], d1[1], qsets[0], sub, debug=True)
        np.testing.assert_array_equal(dbg["cmats"], o["cmats"], err_msg=f"{name}: oracle counts, sub={sub}")
        np.testing.assert_array_equal(rstat[:, 1], o_rstat[:, 1], err_msg=f"{name}: oracle nsnps, sub={sub}")
    # 2: the map on the device is the host planner's
    np.testing.assert_array_equal(E1.boot_pack_map(), pack_sites(d1[1]))


def test_map_is_the_host_planners_on_a_c5_like_replicate(pair):
    from tetrad_amd import bootstrap, synth
    from tetrad_amd.engine import pack_sites
    E0, E1 = pair
    seqarr, _, spans = synth.make_c5_source(T=16, S=5000)
    lidxs, s1, s2 = bootstrap.draw_replicate(len(spans), np.random.default_rng(5))
    S = build_both(E0, E1, (seqarr, spans), lidxs, (s1, s2))
    assert padded(S) == 3 * TILE
    tmpmap = E1.get_data()[1]
    src = E1.boot_pack_map()
    np.testing.assert_array_equal(src, pack_sites(tmpmap))
    q = [synth.random_quartets(16, 400, seed=2)]
    assert_same_rows(rows_of(E0, q), rows_of(E1, q), "c5-like")


# -- 3 ------------------------------------------------------------------------------------------------------------------
def test_packed_set_longer_than_the_natural_one(pair):
    """One 17-site locus drawn 200 times: no two of them share a 32-site word, so the packed set takes 200 words = 6 400
    sites -> 8 192 padded, against 3 410 -> 4 096 natural: sized from the plan, not from the natural length."""
    E0, E1 = pair
    src = ascii_source(10, [17] + [1] * 209, seed=21)
    lidxs = np.array([0] * 200 + list(range(1, 11)), np.int64)
    lidxs = lidxs[np.random.default_rng(4).permutation(len(lidxs))]
    S = build_both(E0, E1, src, lidxs, (7, 9))
    assert S == 200 * 17 + 10 and padded(S) == 2 * TILE
    pk_Sp = E1.site_pack_state()[0]
    assert pk_Sp == 4 * TILE and pk_Sp > padded(S) + TILE
    qsets = quartet_sets(10)
    assert_same_rows(rows_of(E0, qsets), rows_of(E1, qsets), "17-site locus x 200")


# -- 4 ------------------------------------------------------------------------------------------------------------------
def test_life_cycle_on_one_engine(source10):
    from tetrad_amd import synth
    from tetrad_amd._lib import TetradHipError
    from tetrad_amd.engine import QuartetEngine, pack_sites
    seqarr, spans = source10
    q10, q12 = quartet_sets(10), quartet_sets(12)
    variants = ({}, {"wg_min_quartets": 64})

    def fresh_rows(src, lidxs, seeds, qsets):
        with QuartetEngine(0) as F:
            F.set_option("boot_pack", 0)
            F.set_source(*src)
            F.bootstrap(lidxs, *seeds)
            assert not F.site_pack_state()[1]
            return rows_of(F, qsets, variants), F.get_data()

    with QuartetEngine(0) as E:
        E.set_option("boot_pack", 1)
        E.set_source(seqarr, spans)

        def step(src, first, S, qsets, what, packed=True):
            lidxs = draws(src[1], first, S)
            assert E.bootstrap(lidxs, S, S + 1) == S
            sites, used = E.site_pack_state()
            assert used == packed, what
            want, data = fresh_rows(src, lidxs, (S, S + 1), qsets)
            assert_same_rows(want, rows_of(E, qsets, variants), what)
            if packed:
                np.testing.assert_array_equal(E.boot_pack_map(), pack_sites(data[1]), err_msg=what)
            else:
                with pytest.raises(TetradHipError):
                    E.boot_pack_map()
            return sites

        src = (seqarr, spans)
        long_ = step(src, [L[2100], L[2048], L[65]], 3 * TILE + 1, q10, "long")
        short = step(src, [L[100], L[65], L[33]], TILE + 1, q10, "short after long")
        assert short < long_
        grown = step(src, [L[2100]] * 4, 5 * TILE + 1, q10, "outgrows the packed buffers")
        assert grown > padded(long_ + long_ // 8)                 # beyond the head-room of the first allocation
        # tq_set_data with site_pack = 1: its own packed set is current, and it is not a replicate's
        E.set_option("site_pack", 1)
        big = synth.simulate_tmparr(10, 2 * TILE + 5, seed=31, missing=0.15)
        E.set_data(*big)
        assert E.site_pack_state()[1]
        with pytest.raises(TetradHipError):
            E.boot_pack_map()
        with QuartetEngine(0) as F:
            F.set_option("site_pack", 0)
            F.set_data(*big)
            assert_same_rows(rows_of(F, q10, variants), rows_of(E, q10, variants), "tq_set_data between replicates")
        step(src, [L[2047], L[65]], 2 * TILE - 1, q10, "replicate after a packed tq_set_data")
        E.set_option("site_pack", -1)
        # boot_pack switched off: the next replicate is natural and the packed set stale
        E.set_option("boot_pack", 0)
        step(src, [L[2100], L[33]], 2 * TILE + 32, q10, "boot_pack 0", packed=False)
        # site_pack = 0 wins over boot_pack = 1
        E.set_option("boot_pack", 1)
        E.set_option("site_pack", 0)
        step(src, [L[2048], L[33]], 2 * TILE + 31, q10, "site_pack 0", packed=False)
        E.set_option("site_pack", -1)
        step(src, [L[2048], L[33]], 2 * TILE + 31, q10, "site_pack -1 again")
        # another number of taxa
        src12 = layout_source(12, seed=13)
        E.set_source(*src12)
        step(src12, [L[100], L[65], L[33]], TILE + 33, q12, "12 taxa")


# -- 5 ------------------------------------------------------------------------------------------------------------------
def test_readers_of_the_natural_set(pair, source10):
    from itertools import combinations
    E0, E1 = pair
    lidxs = draws(source10[1], [L[2100], L[2048], L[65]], 3 * TILE + 17)
    build_both(E0, E1, source10, lidxs, (3, 5))
    q = quartet_sets(10)[1]
    sq = np.array(list(combinations(range(5), 4)), np.uint32)
    out = []
    for E in (E0, E1):
        E.set_species(np.arange(10, dtype=np.int32) // 2, 5)
        rstat, rscor, flags, dbg = E.resolve_species(sq, debug=True)
        full = E.resolve(q, False, debug=True)
        data = E.get_data()
        out.append([np.array(x) for x in (rstat, rscor, flags, dbg["cmats"], *full[:3], full[3]["cmats"], *data)])
    assert E1.site_pack_state()[1]
    for a, b in zip(*out):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


# -- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_replicates_in_flight(sampler):
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd.replicates import ReplicateRunner
    seqarr, _, spans = synth.make_c5_source(T=16, S=5000)
    got = {}
    for bp in (0, 1):
        rows = got[bp] = {}
        with QuartetEngine(0) as eng:
            eng.set_option("boot_pack", bp)
            runner = ReplicateRunner(eng, seqarr, spans, 400, seed=99, sampler=sampler, ahead=2)
            stats = runner.run(4, True, on_result=lambda k, S, a, b, c: rows.__setitem__(k, (a.copy(), b.copy(), c.copy())))
            runner.close()
            assert eng.site_pack_state()[1] == bool(bp)
        rows["sites"] = stats["sites"]
    assert got[0]["sites"] == got[1]["sites"] and len(got[0]["sites"]) == 4
    for k in range(4):
        for a, b, what in zip(got[0][k], got[1][k], ("rstat", "rscor", "flags")):
            np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"replicate {k}: {what}")


# -- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dense", "rad60"])
def test_automatic_rule(which):
    """boot_pack = -1 packs replicates of the dense c5 source and not of the sparse rad60 one: the decision of the host
    rule (tq_pack_sites with the matrix) on the source's own matrix."""
    from tetrad_amd import bootstrap, synth
    from tetrad_amd.engine import QuartetEngine, pack_sites
    if which == "dense":
        seqarr, tmpmap, spans = synth.make_c5_source()
    else:
        seqarr, tmpmap, spans = synth.make_c5_source(source=synth.radseq_profile("rad60"))
    assert seqarr.shape == (128, 50_000)
    _, pays, est = pack_sites(tmpmap, CODE[seqarr])
    print(which, "estimate", est)
    assert pays == (which == "dense")
    lidxs, s1, s2 = bootstrap.draw_replicate(len(spans), np.random.default_rng(11))
    q = synth.random_quartets(128, 2000, seed=77)
    rows = {}
    for bp in (-1, 0):
        with QuartetEngine(0) as eng:
            eng.set_option("boot_pack", bp)
            eng.set_source(seqarr, spans)
            eng.bootstrap(lidxs, s1, s2)
            assert eng.site_pack_state()[1] == (pays and bp == -1)
            rows[bp] = [np.array(x) for x in eng.resolve(q, True)]
    for a, b, what in zip(rows[0], rows[-1], ("rstat", "rscor", "flags")):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)
