"""GPU: site-pattern class rows against the oracle's count matrices and an independent model (tests/patterns_model.py),
the D accumulation against the host execution and Python floats, and `run_dstat` end to end."""
import ctypes
from itertools import combinations

import numpy as np
import pytest

from conftest import load_golden
import patterns_model as pm

pytestmark = pytest.mark.gpu

GOLDENS = ["tiny_T5_S37", "one_site_T5_S1", "edge_T7_S130", "sparse_T10_S257", "c1_T16_S5000"]


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


@pytest.fixture(scope="module")
def table():
    from tetrad_amd import patterns
    return patterns.class_table()


def all_sets(T):
    return np.array(list(combinations(range(T), 4)), np.uint32)


_REF = {}


def golden_reference(name, sub, oracle, table):
    """(tmparr, tmpmap, sets, classes from the oracle's cmats through the table, classes of the model, nsnps), once."""
    if (name, sub) not in _REF:
        g = load_golden(name)
        sets = all_sets(g["tmparr"].shape[0])
        _, rstat, _, dbg = oracle.new_infer_resolved_quartets(g["tmparr"], g["tmpmap"], sets, sub, debug=True)
        _REF[name, sub] = (g["tmparr"], g["tmpmap"], sets, pm.table_classes(dbg["cmats"][:, 0].reshape(-1, 256), table),
                           pm.model_classes(g["tmparr"], g["tmpmap"], sets, sub), rstat[:, 1].copy())
    return _REF[name, sub]


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(engine, oracle, table, name, sub):
    tmparr, tmpmap, sets, by_table, by_model, nsnps = golden_reference(name, sub, oracle, table)
    engine.set_data(tmparr, tmpmap)
    classes = engine.patterns(sets, sub)
    # the slab index of the issue: flattening 0 of the oracle, row 4 x0 + x1, column 4 x2 + x3
    engine.resolve(sets, sub)
    slab = engine.debug_fetch("cm", len(sets))
    assert np.array_equal(pm.table_classes(slab, table), by_table)
    assert classes.dtype == np.uint32 and classes.shape == (len(sets), 16)
    assert np.array_equal(classes, by_table)
    assert np.array_equal(classes, by_model)
    assert np.array_equal(classes[:, 15], nsnps)
    assert not classes[:, 0].any()


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("Q", [1, 3, 4, 5, 63, 64, 65])
def test_prefix_sizes(engine, oracle, table, Q, sub):
    """Four quartets per wavefront, sixteen per workgroup: sizes around those edges, with a canary behind the rows."""
    import torch
    tmparr, tmpmap, sets, by_table, by_model, _ = golden_reference("c1_T16_S5000", sub, oracle, table)
    engine.set_data(tmparr, tmpmap)
    assert np.array_equal(engine.patterns(sets[:Q], sub), by_model[:Q])
    d_sets = torch.from_numpy(sets[:Q].view(np.int32)).cuda()
    d_out = torch.full((Q + 3, 16), -1, dtype=torch.int32, device="cuda")
    engine.patterns_dev(d_sets.data_ptr(), Q, sub, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:Q], by_table[:Q]) and (out[Q:] == 0xFFFFFFFF).all()


@pytest.fixture(scope="module")
def random21():
    """21 taxa x 300 sites, 20 % missing, loci of 1..6 sites: 5 985 sets, above wg_min_quartets."""
    rng = np.random.default_rng(21)
    T, S = 21, 300
    tmparr = rng.integers(0, 4, size=(T, S)).astype(np.uint8)
    tmparr[:, : S // 2] = tmparr[rng.integers(0, 3, size=T)][:, : S // 2]          # some structure: shared patterns
    tmparr[rng.random((T, S)) < 0.2] = 78
    widths = []
    while sum(widths) < S:
        widths.append(int(rng.integers(1, 7)))
    locus = np.repeat(np.arange(len(widths)), widths)[:S].astype(np.uint32)
    tmpmap = np.stack([locus, np.arange(S, dtype=np.uint32)], axis=1)
    sets = all_sets(T)
    ref = {sub: pm.model_classes(tmparr, tmpmap, sets, sub) for sub in (False, True)}
    return tmparr, tmpmap, sets, ref


@pytest.mark.parametrize("sub", [False, True])
def test_random_matrix_and_batches(engine, random21, sub):
    tmparr, tmpmap, sets, ref = random21
    assert len(sets) == 5985
    engine.set_data(tmparr, tmpmap)
    assert np.array_equal(engine.patterns(sets, sub), ref[sub])
    assert engine.last_scan()[0] != "one_wave"
    engine.set_option("batch", 2048)                                               # three batches
    try:
        assert np.array_equal(engine.patterns(sets, sub), ref[sub])
    finally:
        engine.set_option("batch", 0)


def test_joint_histogram_scan_feeds_the_slab(engine, random21):
    tmparr, tmpmap, sets, ref = random21
    engine.set_data(tmparr, tmpmap)
    engine.set_option("dp_min_quartets", 1024)
    try:
        assert np.array_equal(engine.patterns(sets, False), ref[False])
        assert engine.last_scan()[0] == "dp"
    finally:
        engine.set_option("dp_min_quartets", 0)


def test_other_stream_two_calls(engine, random21):
    import torch
    tmparr, tmpmap, sets, ref = random21
    engine.set_data(tmparr, tmpmap)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
        a = torch.empty((len(sets), 16), dtype=torch.int32, device="cuda")
        b = torch.empty((len(sets), 16), dtype=torch.int32, device="cuda")
        engine.patterns_dev(d_sets.data_ptr(), len(sets), False, a.data_ptr(), st.cuda_stream)
        engine.patterns_dev(d_sets.data_ptr(), len(sets), True, b.data_ptr(), st.cuda_stream)
        st.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), ref[False])
    assert np.array_equal(b.cpu().numpy().view(np.uint32), ref[True])


def test_counts_above_16_bits(engine):
    rng = np.random.default_rng(8)
    S, big = 70_000, 66_000
    tmparr = np.zeros((4, S), np.uint8)
    tmparr[:, :big] = np.array([0, 1, 1, 0], np.uint8)[:, None]                    # class 8, 0110
    for i, s in enumerate(range(big, S)):
        bases = rng.permutation(4)
        tmparr[:, s] = [bases[int(ch)] for ch in pm.STRINGS[1 + i % 14]]
    tmparr = tmparr[:, rng.permutation(S)]
    tmpmap = np.stack([np.arange(S, dtype=np.uint32) // 3, np.arange(S, dtype=np.uint32)], axis=1)
    sets = np.array([[0, 1, 2, 3]], np.uint32)
    engine.set_data(tmparr, tmpmap)
    classes = engine.patterns(sets, False)
    assert np.array_equal(classes, pm.model_classes(tmparr, tmpmap, sets, False))
    assert classes[0, 8] >= big > 65535 and classes[0, 15] == S and classes[0, 1:15].all()


def test_invariant_sites(engine):
    g = load_golden("tiny_T5_S37")
    sets = all_sets(5)
    engine.set_data(g["tmparr"], g["tmpmap"])
    engine.set_option("count_invariant", 1)
    try:
        for sub in (False, True):
            classes = engine.patterns(sets, sub)
            assert np.array_equal(classes, pm.model_classes(g["tmparr"], g["tmpmap"], sets, sub, count_invariant=True))
        assert engine.patterns(sets, False)[:, 0].any()
    finally:
        engine.set_option("count_invariant", 0)


def raw_patterns(engine, sets, sub):
    """tq_patterns into a sentinel-filled array: (return code, the array)."""
    sets = np.ascontiguousarray(sets, dtype=np.uint32).reshape(-1, 4)
    out = np.full((max(1, len(sets)), 16), 0xABABABAB, np.uint32)
    rc = engine._lib.tq_patterns(engine._h, ctypes.c_void_p(sets.ctypes.data), len(sets), int(sub),
                                 ctypes.c_void_p(out.ctypes.data))
    return rc, out


def test_refusals_leave_the_outputs_alone(engine):
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd._lib import TetradHipError
    g = load_golden("edge_T7_S130")
    engine.set_data(g["tmparr"], g["tmpmap"])
    good = all_sets(7)[:6]
    for bad_row, word in (([3, 2, 1, 0], "ascending"), ([0, 1, 2, 2], "ascending"), ([0, 1, 2, 7], ">= T")):
        sets = good.copy()
        sets[4] = bad_row
        rc, out = raw_patterns(engine, sets, False)
        assert rc == -1 and (out == 0xABABABAB).all()
        msg = engine._lib.tq_last_error(engine._h).decode()
        assert "row 4" in msg and word in msg
    with QuartetEngine(0) as fresh:
        rc, out = raw_patterns(fresh, good, False)
        assert rc == -4 and (out == 0xABABABAB).all()
    import torch
    d_sets = torch.from_numpy(good.view(np.int32)).cuda()
    d_out = torch.from_numpy(np.full((len(good) + 1, 16), 0xABABABAB, np.uint32).view(np.int32)).cuda()
    cs = torch.cuda.current_stream().cuda_stream
    for off_sets, off_out in ((4, 0), (0, 4)):              # rows are 16-byte words: a misaligned pointer is refused
        with pytest.raises(TetradHipError) as e:
            engine.patterns_dev(d_sets.data_ptr() + off_sets, len(good) - 1, False, d_out.data_ptr() + off_out, cs)
        assert e.value.code == -1 and "aligned" in str(e.value)
    assert (d_out.cpu().numpy().view(np.uint32) == 0xABABABAB).all()
    for name, value, back in (("scan_method", 2, -1), ("phases", 1, 3), ("phases", 2, 3)):
        engine.set_option(name, value)
        try:
            rc, out = raw_patterns(engine, good, True)
            assert rc == -1 and (out == 0xABABABAB).all()
            assert "diagnostic" in engine._lib.tq_last_error(engine._h).decode()
            with pytest.raises(TetradHipError):
                engine.patterns_dev(d_sets.data_ptr(), len(good), False, d_out.data_ptr(), cs)
            assert (d_out.cpu().numpy().view(np.uint32) == 0xABABABAB).all()
        finally:
            engine.set_option(name, back)
    rc, out = raw_patterns(engine, np.zeros((0, 4), np.uint32), False)
    assert rc == 0 and (out == 0xABABABAB).all()
    assert engine.patterns(np.zeros((0, 4), np.uint32)).shape == (0, 16)
    assert np.array_equal(engine.patterns(good, False), pm.model_classes(g["tmparr"], g["tmpmap"], good, False))


@pytest.mark.parametrize("method", [0, 1])
def test_species(engine, table, method):
    import torch
    from species_model import lineage_data, pooled_factored
    sizes = [3, 1, 4, 2, 2]
    tmparr, tmpmap, sp = lineage_data(sizes, 900, seed=4, missing=0.1, p_within=0.15, left_out=0)
    assert tmparr.shape[0] == 12
    ssets = all_sets(5)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, 5)
    engine.set_option("species_method", method)
    try:
        want = pm.table_classes(pooled_factored(tmparr, sp, 5, ssets)[:, 0].reshape(-1, 256), table)
        assert np.array_equal(engine.patterns_species(ssets), want)
        d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
        d_out = torch.zeros((5, 16), dtype=torch.int32, device="cuda")
        engine.patterns_species_dev(d_sets.data_ptr(), 5, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
        rc = engine._lib.tq_patterns_species(engine._h, ctypes.c_void_p(ssets[::-1].copy().ctypes.data), 5, None)
        assert rc == -1
        bad = ssets.copy()
        bad[2] = [1, 0, 2, 3]
        out = np.full((5, 16), 7, np.uint32)
        rc = engine._lib.tq_patterns_species(engine._h, ctypes.c_void_p(bad.ctypes.data), 5, ctypes.c_void_p(out.ctypes.data))
        assert rc == -1 and (out == 7).all() and "row 2" in engine._lib.tq_last_error(engine._h).decode()
    finally:
        engine.set_option("species_method", -1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("N", [1, 64, 65, 1000])
def test_dstat_accumulate_dev(engine, N):
    import torch
    from tetrad_amd import patterns
    reps, set_of, ia, ib = pm.dstat_case(N)
    M = len(reps[0])
    host = np.zeros((N, 4), np.float64)
    d_acc = torch.zeros((N + 1, 4), dtype=torch.float64, device="cuda")
    d_set_of = torch.from_numpy(set_of.view(np.int32)).cuda()
    d_ia, d_ib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    cs = torch.cuda.current_stream().cuda_stream
    for c in reps:
        patterns.dstat_accumulate(c, set_of, ia, ib, host)
        d_c = torch.from_numpy(c.view(np.int32)).cuda()
        engine.dstat_accumulate_dev(d_c.data_ptr(), M, d_set_of.data_ptr(), d_ia.data_ptr(), d_ib.data_ptr(), N,
                                    d_acc.data_ptr(), cs)
    dev = d_acc.cpu().numpy()
    assert np.array_equal(bits(dev[:N]), bits(host))
    assert np.array_equal(bits(host), bits(np.array(pm.dstat_model(reps, set_of, ia, ib))))
    assert not dev[N].any()


def test_dstat_accumulate_dev_skips_bad_indices(engine):
    """set_of >= n_sets or a class index above 14: the thread returns, its row keeps its bits."""
    import torch
    reps, set_of, ia, ib = pm.dstat_case(65)
    M = len(reps[0])
    set_of, ia, ib = set_of.copy(), ia.copy(), ib.copy()
    set_of[10], ia[20], ib[30] = M, 15, 255
    d_acc = torch.full((65, 4), 2.5, dtype=torch.float64, device="cuda")
    d_c = torch.from_numpy(reps[1].view(np.int32)).cuda()
    d_set_of = torch.from_numpy(set_of.view(np.int32)).cuda()
    d_ia, d_ib = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    engine.dstat_accumulate_dev(d_c.data_ptr(), M, d_set_of.data_ptr(), d_ia.data_ptr(), d_ib.data_ptr(), 65, d_acc.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    got = d_acc.cpu().numpy()
    keep = np.ones(65, bool)
    keep[[10, 20, 30]] = False
    assert (got[~keep] == 2.5).all()
    want = pm.dstat_model([reps[1]], set_of[keep], ia[keep], ib[keep], acc=[[2.5] * 4 for _ in range(int(keep.sum()))])
    assert np.array_equal(bits(got[keep]), bits(np.array(want)))


@pytest.mark.parametrize("sub", [False, True])
def test_run_dstat_end_to_end(sub):
    from tetrad_amd import bootstrap, patterns
    from tetrad_amd.engine import QuartetEngine
    g = load_golden("resample_T7_S300")
    seqarr, spans, tmpmap = g["seqarr"], g["spans"], g["maparr"]
    code = np.full(256, 78, np.uint8)                       # the source matrix itself: A C G T -> 0..3, the rest missing
    code[[ord(ch) for ch in "ACGT"]] = [0, 1, 2, 3]
    tmparr = code[seqarr]
    tests = patterns.tests_with_outgroup(7, 0)
    nboots = 4
    with QuartetEngine(0) as eng:
        res = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, spans, tests, nboots, subsample_snps=sub, seed=5)
        none = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, spans, tests, 0, subsample_snps=sub, seed=5)
    # by hand: the same draws, replicates through the host, the model and Python floats
    sets, set_of, ia, ib = patterns.dstat_tests(tests)
    rng = np.random.default_rng(5)
    reps = []
    with QuartetEngine(0) as eng:
        eng.set_source(seqarr, spans)
        for _ in range(nboots):
            eng.bootstrap(*bootstrap.draw_replicate(len(spans), rng))
            reps.append(pm.model_classes(*eng.get_data(), sets, sub))
    obs = pm.model_classes(tmparr, tmpmap, sets, sub)
    acc = pm.dstat_model(reps, set_of, ia, ib)
    assert len(res) == len(tests) == 60
    D = []
    for t, test in enumerate(tests):
        a, b = int(obs[set_of[t], ia[t]]), int(obs[set_of[t], ib[t]])
        if not sub:
            assert (a, b) == pm.direct_abba_baba(tmparr, test)
        bbaa = int(pm.model_classes(tmparr, tmpmap, [test], sub)[0, 3])
        assert (res["abba"][t], res["baba"][t], res["bbaa"][t], res["nsites"][t]) == (a, b, bbaa, obs[set_of[t], 15])
        D.append((a - b) / (a + b) if a + b else float("nan"))
    assert np.array_equal(bits(res["D"]), bits(D))
    want = np.array(pm.moments_model(D, acc), float)
    assert np.array_equal(res["boot_n"], want[:, 0].astype(np.int64))
    for k, field in enumerate(("boot_mean", "boot_std", "Z"), start=1):
        assert np.array_equal(bits(res[field]), bits(want[:, k])), field
    assert res["boot_n"].max() == nboots and np.isfinite(res["Z"]).any()
    for field in ("abba", "baba", "bbaa", "nsites"):
        assert np.array_equal(none[field], res[field])
    assert np.array_equal(bits(none["D"]), bits(res["D"]))
    assert (none["boot_n"] == 0).all()
    assert np.isnan(none["boot_mean"]).all() and np.isnan(none["boot_std"]).all() and np.isnan(none["Z"]).all()


def test_run_dstat_species():
    """Species tests: the observed columns are those of the pooled counts, the bootstrap columns are filled."""
    from species_model import lineage_data, pooled_factored
    from tetrad_amd import bootstrap as boot, patterns
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap, sp = lineage_data([3, 1, 4, 2, 2], 600, seed=6, missing=0.05, p_within=0.1, left_out=0)
    tmpmap = np.stack([np.arange(600, dtype=np.uint32) // 4, np.arange(600, dtype=np.uint32)], axis=1)
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)].copy()
    seqarr[tmparr > 3] = ord("N")
    tests = patterns.tests_with_outgroup(5, 4)
    with QuartetEngine(0) as eng:
        res = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, boot.get_spans(tmpmap), tests, 3, seed=2, species_of=sp)
    sets, set_of, ia, ib = patterns.dstat_tests(tests)
    want = pm.table_classes(pooled_factored(tmparr, sp, 5, sets)[:, 0].reshape(-1, 256), patterns.class_table())
    assert np.array_equal(res["abba"], want[set_of, ia]) and np.array_equal(res["baba"], want[set_of, ib])
    assert np.array_equal(res["nsites"], want[set_of, 15])
    assert (res["boot_n"] <= 3).all() and res["boot_n"].max() == 3
    with pytest.raises(ValueError):
        patterns.run_dstat(None, tmparr, tmpmap, seqarr, None, tests, 3, subsample_snps=True, species_of=sp)
