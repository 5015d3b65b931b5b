"""GPU: the two forms of the species-mode pooled-count kernel (option "species_method": 0 = VALU, 1 = MFMA) give the
same bits as each other and as the CPU model (tests/species_model.py), including the accumulator drain of the MFMA form
at large S; the automatic choice; and the range refusals (per-row product on the host, zero counts on the device,
at most 255 lineages per species)."""
from itertools import combinations

import numpy as np
import pytest

from species_model import pooled_factored

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
