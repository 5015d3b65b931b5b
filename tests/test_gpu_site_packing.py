"""GPU: option ``site_pack`` -- the subsample-mode scans on the packed layout set (whole loci per lane word, csrc/pack.hpp)
against the same calls on the natural layout: rstat, rscor, flags and the debug count matrices must be BITWISE equal
(the count matrix is a histogram over loci; the layout only changes which lane counts which locus).

Inputs: every golden case that carries a matrix, both modes, sorted and unsorted quartets, batches scanned by the
one-wave kernel and by the cooperative kernels (plane-record and nibble-code form); a matrix with loci longer than a
lane word and longer than a 2048-site step whose counted sites lie deep inside them; 2 000 quartets at the c3 and c4
shapes.  Also: tq_get_data still returns the matrix in its own order, a device-built bootstrap replicate after a packed
tq_set_data is resolved from the natural layout (the packed set is stale then), and the automatic rule takes the packed
set on the dense c3 matrix and not on the sparse rad60 one."""
import numpy as np
import pytest

from conftest import GOLDEN_FULL_CASES, load_golden

pytestmark = pytest.mark.gpu

MATRIX_CASES = GOLDEN_FULL_CASES + ["c1_T16_S5000"]


def resolve_all(eng, q, variants):
    """Rows of every (mode, kernel variant) as one flat list of arrays: debug call (with cmats) and plain call."""
    out = []
    defaults = {"wg_min_quartets": 0, "scan_f4": -1, "order": 1}
    for sub in (True, False):
        for opts in variants:
            for k, v in opts.items():
                eng.set_option(k, v)
            rstat, rscor, flags, dbg = eng.resolve(q, sub, debug=True)
            plain = eng.resolve(q, sub)
            for k in opts:
                eng.set_option(k, defaults[k])
            for a, b in zip((rstat, rscor, flags), plain):
                np.testing.assert_array_equal(a, b, err_msg=f"debug vs plain call, {opts} sub={sub}")
            out += [(f"{opts} sub={sub} {name}", np.array(x)) for name, x in
                    (("rstat", rstat), ("rscor", rscor), ("flags", flags), ("cmats", dbg["cmats"]))]
    return out


def packed_vs_natural(tmparr, tmpmap, quartet_sets, variants):
    from tetrad_amd.engine import QuartetEngine
    rows = {}
    with QuartetEngine(0) as eng:
        for sp in (0, 1):
            eng.set_option("site_pack", sp)
            eng.set_data(tmparr, tmpmap)
            sites, used = eng.site_pack_state()
            assert used == bool(sp) and (sites > 0) == bool(sp), (sp, sites, used)
            rows[sp] = [r for q in quartet_sets for r in resolve_all(eng, q, variants)]
    assert len(rows[0]) == len(rows[1])
    for (what, a), (_, b) in zip(rows[0], rows[1]):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"site_pack 0 vs 1: {what}")


# one-wave kernel (batch below wg_min_quartets), cooperative plane-record kernel, cooperative nibble-code kernel
VARIANTS = ({}, {"wg_min_quartets": 64}, {"wg_min_quartets": 64, "scan_f4": 0}, {"wg_min_quartets": 64, "order": 0})


def quartet_sets(q, seed=3):
    """Sorted and unsorted, at least 64 rows (the cooperative kernels take batches of 64 or more)."""
    q = np.ascontiguousarray(q, dtype=np.uint32)
    if len(q) < 64:
        q = np.concatenate([q] * -(-64 // len(q)))
    srt = q[np.lexsort((q[:, 3], q[:, 2], q[:, 1], q[:, 0]))]
    return [np.ascontiguousarray(srt), np.ascontiguousarray(srt[np.random.default_rng(seed).permutation(len(srt))])]


@pytest.mark.parametrize("case", MATRIX_CASES)
def test_golden_cases_bitwise(case):
    g = load_golden(case)
    packed_vs_natural(g["tmparr"], g["tmpmap"], quartet_sets(g["quartets"]), VARIANTS)


def long_locus_matrix(seed=5):
    """10 taxa; loci of 1-9 sites mixed with loci of 33, 40, 100, 2 100 and 5 000 sites.  In the long loci the first sites are
    missing in most taxa, so the counted site of a quartet lies words -- or steps -- after the locus begins."""
    from tetrad_amd import synth
    rng = np.random.default_rng(seed)
    lens = []
    for big in (33, 5000, 40, 100, 2100, 64, 2048, 37):
        lens += (1 + rng.poisson(3, size=40)).tolist() + [big]
    lens += (1 + rng.poisson(3, size=200)).tolist()
    S = int(np.sum(lens))
    tmparr, _ = synth.simulate_tmparr(10, S, seed=seed, missing=0.15)
    locus = np.repeat(np.arange(len(lens), dtype=np.uint32) * 2 + 3, lens)
    start = 0
    for n in lens:
        if n > 32:
            for t in range(10):
                tmparr[t, start:start + int(rng.integers(0, n))] = 78
        start += n
    tmpmap = np.stack([locus, np.arange(S, dtype=np.uint32)], axis=1)
    return tmparr, tmpmap


def test_long_loci_bitwise(oracle):
    from tetrad_amd import synth
    tmparr, tmpmap = long_locus_matrix()
    q = synth.all_quartets(10)
    packed_vs_natural(tmparr, tmpmap, quartet_sets(q), VARIANTS)
    # and the packed rows are the oracle's (subsample mode)
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        eng.set_option("site_pack", 1)
        eng.set_data(tmparr, tmpmap)
        rstat, rscor, flags, dbg = eng.resolve(q, True, debug=True)
    _, o_rstat, _, o = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q, True, debug=True)
    np.testing.assert_array_equal(dbg["cmats"], o["cmats"])
    np.testing.assert_array_equal(rstat[:, 1], o_rstat[:, 1])


@pytest.mark.parametrize("cfg", ["c3", "c4"])
def test_benchmark_shapes_bitwise(cfg):
    from tetrad_amd import synth
    T, S, _ = synth.CONFIGS[cfg]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS[cfg])
    q = synth.random_quartets(T, 2000, seed=77)
    packed_vs_natural(tmparr, tmpmap, quartet_sets(q), VARIANTS)


def test_large_sorted_batch_bitwise():
    """40 000 c3 quartets: above the device-sort threshold, the shape the benchmark runs at (default options)."""
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    T, S, _ = synth.CONFIGS["c3"]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS["c3"])
    q = synth.random_quartets(T, 40_000, seed=78)
    rows = {}
    with QuartetEngine(0) as eng:
        for sp in (0, 1, -1):
            eng.set_option("site_pack", sp)
            eng.set_data(tmparr, tmpmap)
            assert eng.site_pack_state()[1] == (sp != 0)        # -1: the automatic rule takes the packed set on c3
            rows[sp] = eng.resolve(q, True)
        for sp in (1, -1):
            for a, b, what in zip(rows[0], rows[sp], ("rstat", "rscor", "flags")):
                np.testing.assert_array_equal(np.array(a).view(np.uint8), np.array(b).view(np.uint8), err_msg=f"{sp}: {what}")
        # switched off after the fact: the built set is no longer read; switched on again: it is
        eng.set_option("site_pack", 0)
        assert eng.site_pack_state() == (eng.site_pack_state()[0], False) and eng.site_pack_state()[0] > 0
        eng.set_option("site_pack", -1)
        assert eng.site_pack_state()[1]


def test_automatic_rule_leaves_sparse_data_alone():
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap = synth.radseq_profile("rad60")
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        assert eng.site_pack_state() == (0, False)              # no second set is built


def test_export_returns_the_matrix_in_its_own_order():
    g = load_golden("tree_T12_S2000")
    from tetrad_amd.engine import QuartetEngine
    out = {}
    with QuartetEngine(0) as eng:
        for sp in (0, 1):
            eng.set_option("site_pack", sp)
            eng.set_data(g["tmparr"], g["tmpmap"])
            out[sp] = eng.get_data()
    np.testing.assert_array_equal(out[1][0], g["tmparr"])
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(out[1][1], out[0][1])
    # the same locus runs as the input
    a, b = out[1][1][:, 0], g["tmpmap"][:, 0]
    np.testing.assert_array_equal(a[1:] != a[:-1], b[1:] != b[:-1])


def test_bootstrap_replicate_after_packed_set_data():
    """The device-built replicate keeps the natural layout: the packed set of the earlier tq_set_data is stale and must not be
    read.  Same replicate, same quartets, site_pack 0 against 1."""
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    q = synth.all_quartets(7)
    q = np.concatenate([q] * 2)                                 # 70 rows: the cooperative kernels too
    rows = {}
    for sp in (0, 1):
        with QuartetEngine(0) as eng:
            eng.set_option("site_pack", sp)
            eng.set_data(g["tmparr"], g["tmpmap"])
            assert eng.site_pack_state()[1] == bool(sp)
            eng.set_source(g["seqarr"], g["spans"])
            eng.bootstrap(g["lidxs"], 111, 222)
            assert not eng.site_pack_state()[1]
            rows[sp] = [eng.get_data()[0]]
            for opts in ({}, {"wg_min_quartets": 64}):
                for k, v in opts.items():
                    eng.set_option(k, v)
                rstat, rscor, flags, dbg = eng.resolve(q, True, debug=True)
                rows[sp] += [np.array(rstat), np.array(rscor), np.array(flags), dbg["cmats"]]
            # a fresh tq_set_data after the replicate packs again
            eng.set_data(g["tmparr"], g["tmpmap"])
            assert eng.site_pack_state()[1] == bool(sp)
    for a, b in zip(rows[0], rows[1]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
