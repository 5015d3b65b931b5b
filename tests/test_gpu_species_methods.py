"""GPU: the two forms of the species-mode pooled-count kernel (option "species_method": 0 = VALU, 1 = MFMA) give the
same bits as each other and as the CPU model (tests/species_model.py), including the accumulator drain of the MFMA form
at large S; the automatic choice; and the range refusals (per-row product on the host, zero counts on the device,
at most 255 lineages per species).

Further down: the VALU form at the sizes only it takes (12 to 255 lineages), pooled bins and nsnps with bit 31 set through
every consumer of the count slab, the range rule at its edge, and site counts at the edges of the kernels' site dealing.
All count matrices are compared bit for bit with `species_model.pooled_factored`."""
from itertools import combinations

import numpy as np
import pytest

from species_model import check_rows, lineage_data, pooled_factored, species_counts, spike_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng
        eng.set_option("species_method", -1)


def resolve_with(eng, method, rows):
    eng.set_option("species_method", method)
    try:
        return eng.resolve_species(rows, debug=True)
    finally:
        eng.set_option("species_method", -1)


def assert_same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for k in ("cmats", "svds", "ranks"):
        assert np.array_equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("style", ["random", "radseq", "sizes_1_to_11"])
def test_forms_are_bitwise_equal(engine, style):
    from tetrad_amd import synth
    rng = np.random.default_rng(len(style))
    K = 9
    if style == "sizes_1_to_11":
        sizes = np.array([11, 1, 7, 2, 11, 3, 5, 9, 4])
        sp = rng.permutation(np.repeat(np.arange(K, dtype=np.int32), sizes))
        T = sp.size
        tmparr, tmpmap = synth.simulate_tmparr(T, 7000, seed=4, missing=0.2)
    else:
        T = 40
        sp = rng.permutation(np.concatenate([np.arange(K), rng.integers(0, K, T - K - 2), [-1, -1]])).astype(np.int32)
        if style == "random":
            tmparr, tmpmap = synth.simulate_tmparr(T, 5000, seed=2, missing=0.15)
        else:
            tmparr, tmpmap = synth.simulate_radseq(T, 5000, 3, block=0.5, cell=0.02, hi_frac=0.2, dead_taxa=1)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    rows = np.concatenate([rows, rng.integers(0, K, size=(12, 4)).astype(np.uint32)])
    valu = resolve_with(engine, 0, rows)
    mfma = resolve_with(engine, 1, rows)
    auto = engine.resolve_species(rows, debug=True)
    assert_same(valu, mfma)
    assert_same(auto, mfma)
    assert np.array_equal(mfma[3]["cmats"], pooled_factored(tmparr, sp, K, rows))


def test_bench_shape_forms_equal(engine):
    from tetrad_amd import synth
    T, S, K = 128, 50_000, 32
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    rng = np.random.default_rng(5)
    sp = rng.permutation(np.repeat(np.arange(K, dtype=np.int32), 4))
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)[rng.choice(35960, 3000, replace=False)]
    assert_same(resolve_with(engine, 0, rows), resolve_with(engine, 1, rows))


def test_large_S_drains_and_per_row_range(engine):
    """S = 300 000: each wave of the MFMA form walks more than one drain period.  Species 0 holds 11 lineages, the
    others one: the call's bound (S x 11) is fine, but the row (0, 0, 0, 0) has S x 11^4 >= 2^32."""
    from tetrad_amd import _lib
    rng = np.random.default_rng(9)
    S, K = 300_000, 4
    sp = np.array([0] * 11 + [1, 2, 3], np.int32)
    tmparr = rng.integers(0, 4, size=(sp.size, S)).astype(np.uint8)
    tmparr[rng.random(tmparr.shape) < 0.1] = 78
    engine.set_data(tmparr, np.arange(S, dtype=np.uint32))
    engine.set_species(sp, K)
    rows = np.array([[0, 1, 2, 3], [1, 0, 3, 0], [0, 0, 1, 2]], np.uint32)   # 11, 121 and 121 x S: in range
    valu = resolve_with(engine, 0, rows)
    mfma = resolve_with(engine, 1, rows)
    assert_same(valu, mfma)
    assert np.array_equal(mfma[3]["cmats"], pooled_factored(tmparr, sp, K, rows))
    bad = np.array([[0, 1, 2, 3], [0, 0, 0, 0]], np.uint32)
    with pytest.raises(_lib.TetradHipError, match="lineage product"):
        engine.resolve_species(bad)
    import torch
    dev = torch.device("cuda:0")
    for method in (0, 1):
        engine.set_option("species_method", method)
        try:
            dq = torch.from_numpy(bad.view(np.int32)).to(dev)
            drs = torch.empty((2, 2), dtype=torch.int32, device=dev)
            dsc = torch.empty((2, 3), dtype=torch.float64, device=dev)
            dfl = torch.empty(2, dtype=torch.uint8, device=dev)
            engine.resolve_species_dev(dq.data_ptr(), 2, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr())
            torch.cuda.synchronize()
        finally:
            engine.set_option("species_method", -1)
        st, fl = drs.cpu().numpy().view(np.uint32), dfl.cpu().numpy()
        assert st[0, 1] == valu[0][0, 1] and fl[0] == valu[2][0]
        assert st[1, 1] == 0 and fl[1] & _lib.FLAG_ZERO_DATA


def test_method_choice_and_size_refusals(engine):
    from tetrad_amd import _lib, synth
    T = 300
    tmparr, tmpmap = synth.simulate_tmparr(T, 600, seed=6)
    engine.set_data(tmparr, tmpmap)
    rows = np.array([[0, 1, 2, 3]], np.uint32)
    # a species of 12 lineages: the automatic choice is the VALU form, forcing the MFMA form is refused
    sp = np.array([0] * 12 + [1, 2, 3] + [-1] * (T - 15), np.int32)
    engine.set_species(sp, 4)
    auto = engine.resolve_species(rows, debug=True)
    assert_same(auto, resolve_with(engine, 0, rows))
    engine.set_option("species_method", 1)
    try:
        with pytest.raises(_lib.TetradHipError, match="at most 11 lineages"):
            engine.resolve_species(rows)
    finally:
        engine.set_option("species_method", -1)
    with pytest.raises(_lib.TetradHipError, match="species_method"):
        engine.set_option("species_method", 2)
    # more than 255 lineages in one species
    with pytest.raises(_lib.TetradHipError, match="more than 255 lineages"):
        engine.set_species(np.array([0] * 256 + [1, 2, 3] + [-1] * (T - 259), np.int32), 4)


# -- the VALU form at size ---------------------------------------------------------------------------------------------
def rows_with_repeats(K, sizes, S, rng, extra):
    """All species quartets plus `extra` rows that repeat a species, each within the row's own range rule."""
    rows = [list(q) for q in combinations(range(K), 4)]
    while extra:
        r = rng.integers(0, K, 4)
        r[int(rng.integers(1, 4))] = r[0]
        if S * int(np.prod([sizes[k] for k in r])) < 2**32:
            rows.append(r.tolist())
            extra -= 1
    return np.array(rows, np.uint32)


@pytest.mark.parametrize("sizes, S", [((12, 13, 16, 17, 20), 20_000), ((255, 100, 40, 17, 3, 1), 200)])
@pytest.mark.parametrize("missing, p_within", [(0.0, 0.0), (0.2, 0.02)])
def test_valu_form_at_size(engine, oracle, sizes, S, missing, p_within):
    """Species of 12 to 255 lineages that mostly agree: byte counts up to 255, abc up to 255^3 < 2^24, bins up to
    S x the product of the four sizes.  Only the VALU form takes them."""
    rng = np.random.default_rng([len(sizes), S])
    K = len(sizes)
    tmparr, tmpmap, sp = lineage_data(sizes, S, 31, missing=missing, p_within=p_within)
    assert np.bincount(sp[sp >= 0]).tolist() == list(sizes)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = rows_with_repeats(K, sizes, S, rng, 6)
    cm = pooled_factored(tmparr, sp, K, rows)
    if missing == 0.0:                                  # every site holds each species' whole size in one base
        assert (species_counts(tmparr, sp, K).max(axis=2) == np.array(sizes)[:, None]).all()
    valu = resolve_with(engine, 0, rows)
    auto = engine.resolve_species(rows, debug=True)
    assert np.array_equal(valu[3]["cmats"], cm)
    assert_same(auto, valu)
    check_rows(valu[0], valu[1], valu[2], cm, oracle)
    plain = engine.resolve_species(rows)
    for x, y in zip(plain, valu[:3]):
        assert np.array_equal(x, y)


def test_valu_form_255_lineages_one_site(engine, oracle):
    """S = 1, four species of 255 lineages: one bin of 255^4 = 4 228 250 625 (abc = 255^3, the last product above
    2^31)."""
    sizes = (255, 255, 255, 255, 2, 1)
    K = len(sizes)
    sp = np.repeat(np.arange(K, dtype=np.int32), sizes)
    col = np.zeros(sp.size, np.uint8)
    col[sp == 1] = np.where(np.arange(255) < 128, 0, 3)             # species 1: 128 A, 127 T
    col[(sp == 2) | (sp == 3)] = 1
    col[sp == 4] = [0, 2]
    col[sp == 5] = 3
    rng = np.random.default_rng(6)
    order = rng.permutation(sp.size)
    sp, tmparr = sp[order], np.ascontiguousarray(col[order][:, None])
    engine.set_data(tmparr, np.zeros(1, np.uint32))
    engine.set_species(sp, K)
    rows = np.concatenate([rows_with_repeats(K, sizes, 1, rng, 8), np.array([[0, 0, 2, 2], [0, 0, 3, 2]], np.uint32)])
    cm = pooled_factored(tmparr, sp, K, rows)
    assert int(cm.max()) == 255**4 and int((cm[:, 0].reshape(len(rows), -1) == 255**3 * 128).sum()) > 0
    valu = resolve_with(engine, 0, rows)
    assert np.array_equal(valu[3]["cmats"], cm)
    assert_same(engine.resolve_species(rows, debug=True), valu)
    check_rows(valu[0], valu[1], valu[2], cm, oracle)


def test_automatic_choice_at_11_and_12(engine):
    """The same data with a largest species of 11 and of 12 lineages: the automatic choice gives the forced MFMA form's
    outputs at 11 (the VALU form agrees) and the forced VALU form's at 12, where the MFMA form is refused."""
    from tetrad_amd import _lib
    tmparr, tmpmap, sp12 = lineage_data((12, 3, 2, 5, 1), 3000, 8, missing=0.1, p_within=0.05)
    sp11 = sp12.copy()
    sp11[np.flatnonzero(sp12 == 0)[0]] = -1
    engine.set_data(tmparr, tmpmap)
    rows = rows_with_repeats(5, (11, 3, 2, 5, 1), 3000, np.random.default_rng(1), 5)
    engine.set_species(sp11, 5)
    auto = engine.resolve_species(rows, debug=True)
    assert_same(auto, resolve_with(engine, 1, rows))
    assert_same(auto, resolve_with(engine, 0, rows))
    assert np.array_equal(auto[3]["cmats"], pooled_factored(tmparr, sp11, 5, rows))
    engine.set_species(sp12, 5)
    auto = engine.resolve_species(rows, debug=True)
    assert_same(auto, resolve_with(engine, 0, rows))
    assert np.array_equal(auto[3]["cmats"], pooled_factored(tmparr, sp12, 5, rows))
    with pytest.raises(_lib.TetradHipError, match="at most 11 lineages"):
        resolve_with(engine, 1, rows)


# -- counts and nsnps with bit 31 set ----------------------------------------------------------------------------------
SPIKE_S = 293_000
SPIKE_ROWS = np.array([[0, 1, 2, 3], [0, 2, 1, 3], [3, 2, 1, 0], [0, 0, 2, 2]], np.uint32)


@pytest.fixture(scope="module")
def spike():
    tmparr, sp = spike_data(SPIKE_S)
    cm = pooled_factored(tmparr, sp, 4, SPIKE_ROWS)
    assert int(cm[0].max()) == 2_579_729_559 and int(cm[0, 0].sum(dtype=np.uint64)) == 4_263_722_738
    assert (cm.reshape(4, -1).max(1) >= 2**31).all()
    return tmparr, sp, cm


def species_dev(engine, rows, stream=0):
    """`resolve_species_dev` into byte buffers: (rstat as uint32 -- never through a signed view --, rscor, flags, the
    device tensors for a following device consumer)."""
    import torch
    dev = torch.device("cuda:0")
    Q = rows.shape[0]
    dq = torch.from_numpy(rows.view(np.int32)).to(dev)
    drs = torch.zeros(Q * 8, dtype=torch.uint8, device=dev)
    dsc = torch.empty((Q, 3), dtype=torch.float64, device=dev)
    dfl = torch.empty(Q, dtype=torch.uint8, device=dev)
    engine.resolve_species_dev(dq.data_ptr(), Q, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), stream)
    torch.cuda.synchronize()
    rstat = drs.cpu().numpy().view(np.uint32).reshape(Q, 2)
    return rstat, dsc.cpu().numpy(), dfl.cpu().numpy(), (dq, drs, dsc, dfl)


@pytest.mark.parametrize("svd", ["hqr", "jacobi"])
@pytest.mark.parametrize("method", [0, 1])
def test_bins_and_nsnps_with_bit_31(engine, oracle, spike, method, svd):
    """Four species of 11 copies, S = 293 000: bins up to 2 579 729 559 and nsnps = 4 263 722 738 through the count
    slab, both singular-value engines, the plain, debug and device calls, the TSV formatter and the concordance
    accumulator."""
    import torch
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.distributor import format_tsv_bytes
    tmparr, sp, cm = spike
    engine.set_data(tmparr, np.arange(SPIKE_S, dtype=np.uint32))
    engine.set_species(sp, 4)
    engine.set_option("svd_method", 0 if svd == "jacobi" else 1)
    engine.set_option("species_method", method)
    try:
        rstat, rscor, flags, dbg = engine.resolve_species(SPIKE_ROWS, debug=True)
        plain = engine.resolve_species(SPIKE_ROWS)
        d_rstat, d_rscor, d_flags, (dq, drs, dsc, dfl) = species_dev(engine, SPIKE_ROWS)
    finally:
        engine.set_option("species_method", -1)
        engine.set_option("svd_method", 1)
    assert np.array_equal(dbg["cmats"], cm)
    assert rstat.dtype == np.uint32 and int(rstat[0, 1]) == 4_263_722_738
    check_rows(rstat, rscor, flags, cm, oracle)
    assert np.all(flags == 0) and np.all(np.isfinite(rscor))
    for a, b in ((plain, (rstat, rscor, flags)), ((d_rstat, d_rscor, d_flags), (rstat, rscor, flags))):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # consumers of the rows
    text = format_tsv_bytes(SPIKE_ROWS, rscor, rstat).decode().splitlines()
    assert [ln.split("\t")[8] for ln in text] == [str(int(n)) for n in rstat[:, 1]]
    assert text[0].endswith("\t4263722738")
    tree = "((0,1),2,(3,4));"                 # (0,1 | 2,3) is induced on the edge above (0,1); row 3 repeats a taxon
    acc = Concordance(tree, engine=engine)
    host = Concordance(tree)
    acc.add_dev(dq, drs.view(torch.int32).view(-1, 2), dsc, dfl)
    host.add(SPIKE_ROWS, rscor, rstat, flags)
    want = sum(int(n) for n in rstat[:3, 1])
    assert want > 2**33
    for a in (acc, host):
        r = a.raw()
        assert r["skipped"] == 1 and int(r["edge_counts"][:, 1:5].sum()) == 3
        assert int(r["edge_counts"][:, 5].sum()) == want
    acc.close()


def test_range_rule_at_its_edge(engine, oracle):
    """Four species of 11: 14 641 x 293 352 = 4 294 966 632 < 2^32 is accepted, 14 641 x 293 353 = 4 294 981 273 is
    refused, by the host call and by the device call."""
    import torch
    from tetrad_amd import _lib
    rows = SPIKE_ROWS[:2]
    tmparr, sp = spike_data(293_353)
    assert 14_641 * 293_352 < 2**32 <= 14_641 * 293_353
    ok = np.ascontiguousarray(tmparr[:, :293_352])
    engine.set_data(ok, np.arange(293_352, dtype=np.uint32))
    engine.set_species(sp, 4)
    cm = pooled_factored(ok, sp, 4, rows)
    assert int(cm.max()) >= 2**31
    for method in (0, 1):
        got = resolve_with(engine, method, rows)
        assert np.array_equal(got[3]["cmats"], cm)
        check_rows(got[0], got[1], got[2], cm, oracle)
    d_rstat, d_rscor, d_flags, _ = species_dev(engine, rows)
    assert np.array_equal(d_rstat, got[0]) and np.array_equal(d_rscor, got[1]) and np.array_equal(d_flags, got[2])
    engine.set_data(tmparr, np.arange(293_353, dtype=np.uint32))
    with pytest.raises(_lib.TetradHipError, match="2\\^32"):
        engine.resolve_species(rows)
    with pytest.raises(_lib.TetradHipError, match="2\\^32"):
        species_dev(engine, rows)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n, S, methods", [(16, 65_536, (0,)), (8, 1 << 20, (0, 1))])
def test_row_range_rule_at_equality(engine, n, S, methods):
    """One species of n lineages, three of one: the call's bound (S x n) is far away, but the row (0, 0, 0, 0) has
    S x n^4 = 2^32 exactly.  The host call refuses it; on the device call both forms give it zero counts.  With one
    site fewer the row is in range and exact."""
    import torch
    from tetrad_amd import _lib
    assert S * n**4 == 2**32
    rng = np.random.default_rng(n)
    sp = np.array([0] * n + [1, 2, 3], np.int32)
    tmparr = rng.integers(0, 4, size=(sp.size, S)).astype(np.uint8)
    rows = np.array([[0, 1, 2, 3], [0, 0, 0, 0]], np.uint32)
    engine.set_data(tmparr, np.arange(S, dtype=np.uint32))
    engine.set_species(sp, 4)
    with pytest.raises(_lib.TetradHipError, match="lineage product"):
        engine.resolve_species(rows)
    good = engine.resolve_species(rows[:1])
    for method in methods:
        engine.set_option("species_method", method)
        try:
            st, sc, fl, _ = species_dev(engine, rows)
        finally:
            engine.set_option("species_method", -1)
        assert st[0, 1] == good[0][0, 1] and fl[0] == good[2][0]
        assert st[1, 1] == 0 and fl[1] & _lib.FLAG_ZERO_DATA
    less = np.ascontiguousarray(tmparr[:, 1:])
    engine.set_data(less, np.arange(S - 1, dtype=np.uint32))
    cm = pooled_factored(less, sp, 4, rows)
    assert int(cm[1, 0].sum(dtype=np.uint64)) > 2**31
    for method in methods:
        got = resolve_with(engine, method, rows)
        assert np.array_equal(got[3]["cmats"], cm)
        assert np.array_equal(got[0][:, 1], cm[:, 0].reshape(2, -1).sum(1, dtype=np.uint64).astype(np.uint32))
    torch.cuda.synchronize()


# -- site counts at the edges of the kernels' site dealing -------------------------------------------------------------
SITE_EDGES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 262_080, 262_144, 262_208]


def test_site_count_edges(engine):
    """S below one step (three waves idle), at a group (16 sites) and step (64) boundary +- 1, at four steps +- 1, and
    at one drain period of the MFMA form (4 waves x 1 024 steps x 64 sites) -+ one step: both forms against the model."""
    sizes = (3, 2, 11, 1, 4)
    K = 5
    rng = np.random.default_rng(12)
    sp = rng.permutation(np.concatenate([np.repeat(np.arange(K), sizes), [-1]])).astype(np.int32)
    full = rng.integers(0, 4, size=(sp.size, max(SITE_EDGES))).astype(np.uint8)
    full[rng.random(full.shape) < 0.1] = 78
    rows = rows_with_repeats(K, sizes, max(SITE_EDGES), rng, 5)
    assert len(rows) == 10
    for S in SITE_EDGES:
        tmparr = np.ascontiguousarray(full[:, full.shape[1] - S:])      # the last S sites: every S ends differently
        engine.set_data(tmparr, np.arange(S, dtype=np.uint32))
        engine.set_species(sp, K)
        cm = pooled_factored(tmparr, sp, K, rows)
        valu = resolve_with(engine, 0, rows)
        mfma = resolve_with(engine, 1, rows)
        assert np.array_equal(valu[3]["cmats"], cm), S
        assert np.array_equal(mfma[3]["cmats"], cm), S
        assert_same(valu, mfma)
        assert np.array_equal(valu[0][:, 1], cm[:, 0].reshape(len(rows), -1).sum(1, dtype=np.uint64).astype(np.uint32)), S
