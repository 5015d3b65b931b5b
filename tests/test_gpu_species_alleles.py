"""GPU: species mode from both alleles of IUPAC genotypes (option "species_alleles") and the
bootstrap loop for species trees.  The species table is built by `tq_species_allele_table_kernel` straight from the
source matrix through the resident replicate's site map; every count matrix is compared bit for bit with the NumPy
model (tests/species_alleles_model.py: two haplotype rows per sample through `species_model.pooled_factored`)."""
from itertools import combinations

import numpy as np
import pytest

from species_alleles_model import (LOOP_K, LOOP_NBOOTS, LOOP_SEED, haplotypes, loop_draws, loop_source, pooled_alleles,
                                   replicate_columns)
from species_model import check_rows, parse_tips_newick, pooled_factored

pytestmark = pytest.mark.gpu

ASCII = np.array([65, 67, 71, 84], np.uint8)
TWO_BASE = np.array([82, 75, 83, 89, 87, 77], np.uint8)


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


class alleles:
    """`with alleles(engine, method):` the species calls inside run in allele mode under the given kernel form."""

    def __init__(self, eng, method=-1, on=1):
        self.eng, self.method, self.on = eng, method, on

    def __enter__(self):
        self.eng.set_option("species_method", self.method)
        self.eng.set_option("species_alleles", self.on)

    def __exit__(self, *exc):
        self.eng.set_option("species_alleles", 0)
        self.eng.set_option("species_method", -1)


def load(eng, seqarr, spans, sp, K):
    """Source, the original matrix as the resident replicate, the map (in this order: the map's T is checked against
    the resident data)."""
    from tetrad_amd.bootstrap import identity_replicate
    eng.set_source(seqarr, spans)
    identity_replicate(eng)
    eng.set_species(sp, K)


def random_source(T, S0, rng, ambiguous=0.15, missing=0.1):
    seqarr = ASCII[rng.integers(0, 4, size=(T, S0))]
    amb = rng.random(seqarr.shape) < ambiguous
    seqarr[amb] = rng.choice(TWO_BASE, size=int(amb.sum()))
    seqarr[rng.random(seqarr.shape) < missing] = 78
    return seqarr


def one_site_spans(S0):
    return np.stack([np.arange(S0), np.arange(S0) + 1], axis=1).astype(np.int64)


def species_dev(eng, rows, stream=None):
    """`resolve_species_dev` on `stream` (a torch stream; None = the current one): (rstat u32, rscor, flags)."""
    import torch
    dev = torch.device("cuda:0")
    Q = rows.shape[0]
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        dq = torch.from_numpy(rows.view(np.int32)).to(dev)
        drs = torch.zeros(Q * 8, dtype=torch.uint8, device=dev)
        dsc = torch.empty((Q, 3), dtype=torch.float64, device=dev)
        dfl = torch.empty(Q, dtype=torch.uint8, device=dev)
        eng.resolve_species_dev(dq.data_ptr(), Q, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    return drs.cpu().numpy().view(np.uint32).reshape(Q, 2), dsc.cpu().numpy(), dfl.cpu().numpy()


def assert_same(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for k in ("cmats", "svds", "ranks"):
        assert np.array_equal(a[3][k], b[3][k]), k


# -- 1. matrices equal the model ---------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 5, 1, 4)


@pytest.fixture(scope="module")
def main_case():
    """T = 17 (species of 1, 2, 3, 5, 1, 4 samples and one sample left out) taken from a simulated 6 x 5 data set,
    S0 = 3 000: loci of 1 to 9 sites, one of 40 and one of 2 100; 15 % two-base codes, about 10 % missing."""
    from tetrad_amd import synth
    K, S0 = len(SIZES), 3000
    tmparr, _, sp30, _ = synth.simulate_species(K, 5, S0, seed=15, missing=0.10)
    rng = np.random.default_rng(15)
    keep, sp = [], []
    for k, n in enumerate(SIZES):
        keep += list(np.flatnonzero(sp30 == k)[:n])
        sp += [k] * n
    keep.append(int(np.flatnonzero(sp30 == 0)[-1]))                 # one sample in no species
    sp.append(-1)
    order = rng.permutation(len(keep))
    tmparr, sp = np.ascontiguousarray(tmparr[np.array(keep)[order]]), np.array(sp, np.int32)[order]
    widths = [40, 2100]
    while sum(widths) < S0:
        widths.append(int(min(rng.integers(1, 10), S0 - sum(widths))))
    widths = np.array(widths)[rng.permutation(len(widths))]
    assert widths.sum() == S0 and widths.min() == 1 and sorted(widths)[-2:] == [40, 2100]
    tmpmap = np.stack([np.repeat(np.arange(len(widths)), widths), np.arange(S0)], axis=1).astype(np.uint32)
    seqarr, _, spans = synth.make_c5_source(source=(tmparr, tmpmap), ambiguous=0.15)
    assert spans.shape[0] == len(widths) and 0.08 < (seqarr == 78).mean() < 0.12
    assert np.isin(seqarr, TWO_BASE).mean() > 0.1
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    rows = np.concatenate([rows, rng.integers(0, K, size=(10, 4)).astype(np.uint32)])
    rows[15:, 1] = rows[15:, 0]                                     # ten rows that repeat a species
    return seqarr, spans, sp, K, rows


@pytest.mark.parametrize("draw", ["identity", "draw1", "draw2"])
def test_matrices_equal_the_model(engine, oracle, main_case, draw):
    from tetrad_amd import _lib
    seqarr, spans, sp, K, rows = main_case
    load(engine, seqarr, spans, sp, K)
    nloci = spans.shape[0]
    if draw == "identity":
        lidxs = np.arange(nloci)
    else:
        lidxs = np.random.default_rng(len(draw) + int(draw[-1])).integers(0, nloci, nloci)
        engine.bootstrap(lidxs, 5, 6)
    cm = pooled_alleles(seqarr, sp, K, rows, cols=replicate_columns(spans, lidxs))
    assert cm[:, 0].reshape(len(rows), -1).sum(1).min() > 0
    bad = np.concatenate([rows, np.array([[0, 1, 2, K]], np.uint32)])
    for method in (0, 1):
        with alleles(engine, method):
            rstat, rscor, flags, dbg = engine.resolve_species(rows, debug=True)
            d_rstat, d_rscor, d_flags = species_dev(engine, bad)
        assert np.array_equal(dbg["cmats"], cm), method
        check_rows(rstat, rscor, flags, cm, oracle)
        assert np.array_equal(d_rstat[:-1], rstat) and np.array_equal(d_rscor[:-1], rscor)
        assert np.array_equal(d_flags[:-1], flags)
        assert d_flags[-1] & _lib.FLAG_BAD_INDEX and d_rstat[-1, 1] == 0


def test_site_count_edges(engine):
    """One-site loci, S0 at a 32-site word and a 2 048-site tile -+ 1: the pad sites of the table are 0."""
    sizes = (3, 2, 5, 1)
    rng = np.random.default_rng(3)
    sp = rng.permutation(np.concatenate([np.repeat(np.arange(4), sizes), [-1]])).astype(np.int32)
    full = random_source(sp.size, 2049, rng)
    rows = np.array([[0, 1, 2, 3], [3, 1, 0, 2], [0, 0, 1, 2], [2, 3, 3, 2], [1, 1, 1, 1]], np.uint32)
    for S0 in (1, 31, 32, 33, 2047, 2048, 2049):
        seqarr = np.ascontiguousarray(full[:, full.shape[1] - S0:])
        load(engine, seqarr, one_site_spans(S0), sp, 4)
        cm = pooled_alleles(seqarr, sp, 4, rows)
        for method in (0, 1):
            with alleles(engine, method):
                rstat, _, _, dbg = engine.resolve_species(rows, debug=True)
            assert np.array_equal(dbg["cmats"], cm), (S0, method)
            assert np.array_equal(rstat[:, 1], cm[:, 0].reshape(len(rows), -1).sum(1, dtype=np.uint64).astype(np.uint32))


# -- 2. the same bits as the path that already exists ------------------------------------------------------------------
def test_same_bits_as_haplotype_rows_through_set_data(engine, main_case):
    """Allele mode on the original matrix against the lineage path fed with the model's haplotype rows (2T samples, the
    map repeated): every output of both forms, bit for bit."""
    seqarr, spans, sp, K, rows = main_case
    load(engine, seqarr, spans, sp, K)
    got = {}
    for method in (0, 1):
        with alleles(engine, method):
            got[method] = engine.resolve_species(rows, debug=True)
    hap = haplotypes(seqarr)
    engine.set_data(hap, np.repeat(np.arange(spans.shape[0]), spans[:, 1] - spans[:, 0]).astype(np.uint32))
    engine.set_species(np.repeat(sp, 2), K)
    for method in (0, 1):
        with alleles(engine, method, on=0):
            assert_same(got[method], engine.resolve_species(rows, debug=True))
    assert_same(got[0], got[1])


# -- 3. the coin is out ------------------------------------------------------------------------------------------------
def test_seed_ambig_has_no_influence(engine, main_case):
    seqarr, spans, sp, K, rows = main_case
    load(engine, seqarr, spans, sp, K)
    lidxs = np.random.default_rng(8).integers(0, spans.shape[0], spans.shape[0])
    on, off = [], []
    for seed_ambig in (1, 2):
        engine.bootstrap(lidxs, 4, seed_ambig)
        with alleles(engine):
            on.append(engine.resolve_species(rows, debug=True))
        off.append(engine.resolve_species(rows, debug=True))
    assert_same(on[0], on[1])
    assert not np.array_equal(off[0][3]["cmats"], off[1][3]["cmats"])
    assert np.array_equal(on[0][3]["cmats"], pooled_alleles(seqarr, sp, K, rows, cols=replicate_columns(spans, lidxs)))


# -- 4. table life cycle -----------------------------------------------------------------------------------------------
def test_table_life_cycle(engine, main_case):
    import torch
    seqarr, spans, sp, K, rows = main_case
    load(engine, seqarr, spans, sp, K)
    rng = np.random.default_rng(21)
    nloci = spans.shape[0]
    with alleles(engine):
        for rep in range(2):                            # two replicates in a row: no stale table
            lidxs = rng.integers(0, nloci, nloci)
            engine.bootstrap(lidxs, rep, rep)
            dbg = engine.resolve_species(rows, debug=True)[3]
            cm = pooled_alleles(seqarr, sp, K, rows, cols=replicate_columns(spans, lidxs))
            assert np.array_equal(dbg["cmats"], cm), f"replicate {rep}: stale species table"
    # the option toggled 1 -> 0 -> 1 on one replicate
    with alleles(engine):
        first = engine.resolve_species(rows, debug=True)
    lineage = engine.resolve_species(rows, debug=True)
    assert np.array_equal(lineage[3]["cmats"], pooled_factored(engine.get_data()[0], sp, K, rows))
    with alleles(engine):
        again = engine.resolve_species(rows, debug=True)
        assert_same(first, again)
        assert np.array_equal(again[3]["cmats"], cm)
        # a device call on a second stream, right after a replicate enqueued on another one
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        lidxs = rng.integers(0, nloci, nloci)
        engine.bootstrap(lidxs, 7, 7, s1.cuda_stream)
        d_rstat, d_rscor, d_flags = species_dev(engine, rows, s2)
        host = engine.resolve_species(rows, debug=True)
    assert np.array_equal(host[3]["cmats"], pooled_alleles(seqarr, sp, K, rows, cols=replicate_columns(spans, lidxs)))
    assert np.array_equal(d_rstat, host[0]) and np.array_equal(d_rscor, host[1]) and np.array_equal(d_flags, host[2])


# -- 5. form choice and bounds -----------------------------------------------------------------------------------------
def test_form_choice_at_5_and_6_samples(engine):
    from tetrad_amd import _lib
    rng = np.random.default_rng(5)
    sp6 = np.array([0] * 6 + [1, 1, 2, 3, 3, 3], np.int32)
    sp5 = sp6.copy()
    sp5[0] = -1
    seqarr = random_source(sp6.size, 700, rng)
    rows = np.array([[0, 1, 2, 3], [0, 0, 1, 3], [3, 2, 1, 0]], np.uint32)
    load(engine, seqarr, one_site_spans(700), sp5, 4)           # 10 lineages: 10 x 10 = 100 <= 127
    with alleles(engine, 0):
        valu = engine.resolve_species(rows, debug=True)
    assert np.array_equal(valu[3]["cmats"], pooled_alleles(seqarr, sp5, 4, rows))
    for method in (-1, 1):
        with alleles(engine, method):
            assert_same(valu, engine.resolve_species(rows, debug=True))
    engine.set_species(sp6, 4)                                  # 12 lineages: the VALU form only
    with alleles(engine, 0):
        valu = engine.resolve_species(rows, debug=True)
    assert np.array_equal(valu[3]["cmats"], pooled_alleles(seqarr, sp6, 4, rows))
    with alleles(engine):
        assert_same(valu, engine.resolve_species(rows, debug=True))
    with alleles(engine, 1):
        with pytest.raises(_lib.TetradHipError, match="at most 11 lineages"):
            engine.resolve_species(rows)
        with pytest.raises(_lib.TetradHipError, match="at most 11 lineages"):
            species_dev(engine, rows)
    # with the option off the same map is within the MFMA form's bound (6 lineages)
    with alleles(engine, 1, on=0):
        engine.resolve_species(rows)


def eight_by_four(S0):
    """T = 32, every cell 'A' except: sample 0 is 'M' (C / A) and samples 24..31 are 'C' at every site."""
    seqarr = np.full((32, S0), 65, np.uint8)
    seqarr[0] = 77
    seqarr[24:] = 67
    return seqarr


def wide_spans(S0, width):
    assert S0 % width == 0
    return np.stack([np.arange(0, S0, width), np.arange(0, S0, width) + width], axis=1).astype(np.int64)


def test_range_rule_in_lineages(engine):
    """Four species of 8 samples are 16 lineages each (product 65 536): S = 65 535 is accepted and exact, with a bin of
    15 x 16^3 x 65 535 = 4 026 470 400 >= 2^31; S = 65 536 is refused by the host and the device call.  A species of 8
    samples and three of one: the call's bound is far away, the row (0, 0, 0, 0) has 16^4 x 65 536 = 2^32."""
    from tetrad_amd import _lib
    rows = np.array([[0, 1, 2, 3], [3, 0, 2, 1]], np.uint32)
    four = (np.arange(32) // 8).astype(np.int32)
    one = np.array([0] * 8 + [1, 2, 3] + [-1] * 21, np.int32)
    rep = np.array([[0, 1, 2, 3], [0, 0, 0, 0]], np.uint32)
    # S = 65 535
    seqarr = eight_by_four(65_535)
    load(engine, seqarr, wide_spans(65_535, 257), four, 4)
    cm = pooled_alleles(seqarr, four, 4, rows)
    assert int(cm.max()) == 15 * 16**3 * 65_535 >= 2**31
    with alleles(engine):
        rstat, rscor, flags, dbg = engine.resolve_species(rows, debug=True)
        d_rstat, d_rscor, d_flags = species_dev(engine, rows)
    assert np.array_equal(dbg["cmats"], cm)
    assert np.array_equal(rstat[:, 1], cm[:, 0].reshape(2, -1).sum(1, dtype=np.uint64).astype(np.uint32))
    assert np.array_equal(d_rstat, rstat) and np.array_equal(d_rscor, rscor) and np.array_equal(d_flags, flags)
    # ... where the row (0, 0, 0, 0) of the other map is in range, and not empty
    engine.set_species(one, 4)
    cm1 = pooled_alleles(seqarr, one, 4, rep)
    assert int(cm1[1, 0].sum(dtype=np.uint64)) > 0
    with alleles(engine):
        assert np.array_equal(engine.resolve_species(rep, debug=True)[3]["cmats"], cm1)
    # S = 65 536
    seqarr = eight_by_four(65_536)
    load(engine, seqarr, wide_spans(65_536, 256), four, 4)
    with alleles(engine):
        with pytest.raises(_lib.TetradHipError, match="2\\^32"):
            engine.resolve_species(rows)
        with pytest.raises(_lib.TetradHipError, match="2\\^32"):
            species_dev(engine, rows)
    engine.resolve_species(rows)                         # 8^4 x 65 536 = 2^28: in range with the option off
    engine.set_species(one, 4)
    with alleles(engine):
        with pytest.raises(_lib.TetradHipError, match="lineage product"):
            engine.resolve_species(rep)
        good = engine.resolve_species(rep[:1])
        for method in (0, -1):
            engine.set_option("species_method", method)
            st, sc, fl = species_dev(engine, rep)
            assert st[0, 1] == good[0][0, 1] > 0 and fl[0] == good[2][0]
            assert st[1, 1] == 0 and fl[1] & _lib.FLAG_ZERO_DATA
    off = engine.resolve_species(rep)                    # the same row in lineages of one per sample: 8^4 x 65 536
    assert off[0][1, 1] > 0 and not off[2][1] & _lib.FLAG_ZERO_DATA


def test_row_range_rule_in_both_forms(engine):
    """A species of 4 samples (8 lineages, within the MFMA form's bound) and three of one at S = 2^20: the row
    (0, 0, 0, 0) has 8^4 x 2^20 = 2^32 in lineages and gets zero counts from both kernels, while with one lineage per
    sample (4^4 x 2^20 = 2^28) it is an ordinary row."""
    from tetrad_amd import _lib
    S0 = 1 << 20
    rng = np.random.default_rng(20)
    sp = np.array([0, 0, 0, 0, 1, 2, 3], np.int32)
    seqarr = random_source(7, S0, rng)
    rep = np.array([[0, 1, 2, 3], [0, 0, 0, 0]], np.uint32)
    load(engine, seqarr, wide_spans(S0, 4096), sp, 4)
    with alleles(engine):
        with pytest.raises(_lib.TetradHipError, match="lineage product"):
            engine.resolve_species(rep)
        good = engine.resolve_species(rep[:1])
        for method in (0, 1):
            engine.set_option("species_method", method)
            st, sc, fl = species_dev(engine, rep)
            assert st[0, 1] == good[0][0, 1] > 0 and fl[0] == good[2][0]
            assert st[1, 1] == 0 and fl[1] & _lib.FLAG_ZERO_DATA
    off = engine.resolve_species(rep)
    assert off[0][1, 1] > 0 and not off[2][1] & _lib.FLAG_ZERO_DATA


def test_at_most_127_samples_per_species(engine):
    from tetrad_amd import _lib
    rng = np.random.default_rng(127)
    seqarr = random_source(131, 50, rng, missing=0.02)
    rows = np.array([[0, 1, 2, 3], [0, 0, 1, 2]], np.uint32)
    sp128 = np.array([0] * 128 + [1, 2, 3], np.int32)
    sp127 = sp128.copy()
    sp127[5] = -1
    load(engine, seqarr, one_site_spans(50), sp127, 4)
    with alleles(engine):
        dbg = engine.resolve_species(rows, debug=True)[3]
    cm = pooled_alleles(seqarr, sp127, 4, rows)
    assert np.array_equal(dbg["cmats"], cm)
    engine.set_species(sp128, 4)
    with alleles(engine):
        with pytest.raises(_lib.TetradHipError, match="at most 127 samples"):
            engine.resolve_species(rows)
        with pytest.raises(_lib.TetradHipError, match="at most 127 samples"):
            species_dev(engine, rows)
    engine.resolve_species(rows)                         # 128 lineages of one per sample are fine


# -- 6. refusals leave the context usable ------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    from tetrad_amd import _lib
    from tetrad_amd.bootstrap import identity_replicate
    from tetrad_amd.engine import QuartetEngine
    rng = np.random.default_rng(6)
    sp = np.array([0, 0, 1, 2, 2, 3, 3, 3, -1], np.int32)
    seqarr = random_source(9, 300, rng)
    spans = wide_spans(300, 5)
    rows = np.array([[0, 1, 2, 3], [2, 2, 0, 3]], np.uint32)
    cm = pooled_alleles(seqarr, sp, 4, rows)
    tmparr = haplotypes(seqarr)[::2].copy()
    with QuartetEngine(0) as eng:
        def valid():
            with alleles(eng):
                assert np.array_equal(eng.resolve_species(rows, debug=True)[3]["cmats"], cm)

        eng.set_data(tmparr, np.arange(300, dtype=np.uint32))
        eng.set_species(sp, 4)
        with alleles(eng):                                           # no source
            with pytest.raises(_lib.TetradHipError, match="needs the IUPAC source"):
                eng.resolve_species(rows)
        assert np.array_equal(eng.resolve_species(rows, debug=True)[3]["cmats"], pooled_factored(tmparr, sp, 4, rows))
        eng.set_source(seqarr, spans)
        with alleles(eng):                                           # a source, but the resident data are tq_set_data's
            with pytest.raises(_lib.TetradHipError, match="built by tq_bootstrap"):
                eng.resolve_species(rows)
        identity_replicate(eng)
        valid()
        eng.set_data(tmparr, np.arange(300, dtype=np.uint32))        # tq_set_data after a replicate
        with alleles(eng):
            with pytest.raises(_lib.TetradHipError, match="built by tq_bootstrap"):
                eng.resolve_species(rows)
            with pytest.raises(_lib.TetradHipError, match="built by tq_bootstrap"):
                species_dev(eng, rows)
        identity_replicate(eng)
        valid()
        eng.set_source(seqarr, spans)                                # a new source without a replicate of it
        with alleles(eng):
            with pytest.raises(_lib.TetradHipError, match="built by tq_bootstrap"):
                eng.resolve_species(rows)
        identity_replicate(eng)
        valid()
        with pytest.raises(_lib.TetradHipError, match="species_alleles must be"):
            eng.set_option("species_alleles", 2)
        with pytest.raises(_lib.TetradHipError, match="species_alleles must be"):
            eng.set_option("species_alleles", -1)
        valid()


# -- 7. per-sample use -------------------------------------------------------------------------------------------------
def test_every_sample_its_own_species(engine):
    """`species_of = arange(T)` on a source without ambiguity codes: every sample is two equal lineages, so each matrix
    is 16 x the full-mode matrix of the sample quartet on the same replicate."""
    from tetrad_amd import synth
    T = 24
    tmparr, tmpmap = synth.simulate_tmparr(T, 4000, seed=9)
    seqarr, _, spans = synth.make_c5_source(source=(tmparr, tmpmap), ambiguous=0.0)
    load(engine, seqarr, spans, np.arange(T, dtype=np.int32), T)
    engine.bootstrap(np.random.default_rng(1).integers(0, spans.shape[0], spans.shape[0]), 2, 3)
    q = synth.random_quartets(T, 2000, seed=3)
    rstat, rscor, flags, dbg = engine.resolve(q, subsample_snps=False, debug=True)
    with alleles(engine):
        a_rstat, a_rscor, a_flags, a_dbg = engine.resolve_species(q, debug=True)
    assert np.array_equal(a_dbg["cmats"].astype(np.uint64), 16 * dbg["cmats"].astype(np.uint64))
    ok = ((flags | a_flags) & 3) == 0
    assert ok.sum() > 1900 and np.array_equal(a_rstat[ok, 0], rstat[ok, 0])


# -- 8. the loop -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_case():
    return loop_source()


@pytest.mark.parametrize("nquartets", [0, 40])
def test_bootstrap_species_trees(engine, loop_case, nquartets):
    """K = 8 species x 3 samples, S0 = 6 000, 6 replicates.  The trees equal those of the same draws and calls made by
    hand; both supertree back ends return the same strings; one seed gives one result; the majority-rule tree holds
    every split of the generating species tree.  That the case allows this was checked on the CPU model alone (model
    matrices -> oracle scores -> `infer_supertree_exact`): `test_species_alleles_cpu.py::
    test_loop_parameters_recover_the_species_tree` finds all five splits in every one of the six replicate trees, for
    all 70 species quartets and for 40 sampled ones."""
    from tetrad_amd import qmc, species
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.consensus import Consensus
    seqarr, spans, sp, true_nwk = loop_case
    names = [f"clade{k}" for k in range(LOOP_K)]
    smap = species.SpeciesMap(sp, names)
    with Consensus(LOOP_K) as cons:
        dev = species.bootstrap_species_trees(engine, seqarr, spans, smap, LOOP_NBOOTS, nquartets=nquartets,
                                              seed=LOOP_SEED, consensus=cons)
        host = species.bootstrap_species_trees(engine, seqarr, spans, smap, LOOP_NBOOTS, nquartets=nquartets,
                                               seed=LOOP_SEED, supertree="host")
        again = species.bootstrap_species_trees(engine, seqarr, spans, smap, LOOP_NBOOTS, nquartets=nquartets,
                                                rng=np.random.default_rng(LOOP_SEED))
        assert len(dev) == LOOP_NBOOTS and dev == host == again
        # the same draws and calls by hand
        engine.set_source(seqarr, spans)
        hand = []
        for k, (lidxs, s1, s2, sq) in enumerate(loop_draws(spans.shape[0], nquartets)):
            assert sq.shape == (nquartets or 70, 4)
            engine.bootstrap(lidxs, s1, s2)
            engine.set_species(sp, LOOP_K)
            with alleles(engine):
                rstat, rscor, flags = engine.resolve_species(sq)
            hand.append(qmc.infer_supertree_exact(sq, rscor, rstat, LOOP_K, seed=k, flags=flags))
        assert dev == hand
        assert cons.ntrees == LOOP_NBOOTS
        major = cons.tree(0.5)
        named = qmc.relabel_tree(major, names)
        _, T, tips = newick_to_parent(named, names)
        assert T == LOOP_K and all(n in named for n in names)
        true_splits, _ = parse_tips_newick(true_nwk)
        got_splits, got_tips = parse_tips_newick(major)
        assert got_tips == frozenset(range(LOOP_K)) and len(true_splits) == LOOP_K - 3
        assert true_splits <= got_splits
    # the original matrix first, on request; the option is off again afterwards
    with_orig = species.bootstrap_species_trees(engine, seqarr, spans, smap, 2, nquartets=nquartets, seed=LOOP_SEED,
                                                include_original=True)
    assert len(with_orig) == 3 and with_orig[1:] == dev[:2]
    engine.set_data(haplotypes(seqarr)[::2].copy(), np.arange(seqarr.shape[1], dtype=np.uint32))
    engine.resolve_species(species.species_quartets(LOOP_K))     # the lineage path: not refused, so the option is 0
