"""GPU: species-tree mode -- pooled count matrices of species quartets against the CPU model
(tests/species_model.py, pinned to the oracle's count function), the identity map against `resolve`, the bench shape
against the engine's own lineage matrices, the table after a bootstrap replicate, the device entry point on two
streams, the refusals, and a species tree end to end."""
from itertools import combinations

import numpy as np
import pytest

from species_model import check_rows, parse_tips_newick, pooled_factored, quartet_topology

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as eng:
        yield eng


def random_map(T, K, rng, left_out=2):
    sp = np.concatenate([np.arange(K), rng.integers(0, K, size=T - K - left_out), np.full(left_out, -1)])
    return rng.permutation(sp).astype(np.int32)


@pytest.mark.parametrize("style", ["random", "radseq"])
def test_pooled_matrices_equal_the_model(engine, oracle, style):
    from tetrad_amd import synth
    rng = np.random.default_rng(11)
    T, S, K = 40, 5000, 9
    if style == "random":
        tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=5, missing=0.15)
    else:
        tmparr, tmpmap = synth.simulate_radseq(T, S, 6, block=0.4, cell=0.02, hi_frac=0.2, dead_taxa=1)
    sp = random_map(T, K, rng)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    rows = np.concatenate([rows, rng.integers(0, K, size=(10, 4)).astype(np.uint32)])   # repeated species too
    rstat, rscor, flags, dbg = engine.resolve_species(rows, debug=True)
    cm = pooled_factored(tmparr, sp, K, rows)
    assert np.array_equal(dbg["cmats"], cm)
    check_rows(rstat, rscor, flags, cm, oracle)
    # the plain call gives the same rows
    r2, s2, f2 = engine.resolve_species(rows)
    assert np.array_equal(r2, rstat) and np.array_equal(s2, rscor) and np.array_equal(f2, flags)


def test_identity_map_equals_resolve(engine):
    from tetrad_amd import synth
    T = 24
    tmparr, tmpmap = synth.simulate_tmparr(T, 4000, seed=9)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(np.arange(T, dtype=np.int32), T)
    q = synth.random_quartets(T, 5000, seed=3)
    a = engine.resolve(q, subsample_snps=False)
    b = engine.resolve_species(q)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_bench_shape_equals_summed_lineage_matrices(engine):
    """K = 32 species x 4 lineages, S = 50 000: 200 species quartets against the engine's own count matrices of
    their 51 200 lineage quartets, summed."""
    from tetrad_amd import synth
    T, S, K, n = 128, 50_000, 32, 4
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    rng = np.random.default_rng(1)
    sp = rng.permutation(np.repeat(np.arange(K, dtype=np.int32), n))
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)[rng.choice(35960, 200, replace=False)]
    _, _, _, dbg = engine.resolve_species(rows, debug=True)
    mem = [np.flatnonzero(sp == k) for k in range(K)]
    per = n ** 4
    want = np.zeros((len(rows), 3, 16, 16), np.uint64)
    step = 16                                          # species rows per debug batch (16 x 256 x 3 KB)
    for r0 in range(0, len(rows), step):
        lin = []
        for sq in rows[r0:r0 + step]:
            g = np.stack(np.meshgrid(*(mem[k] for k in sq), indexing="ij"), axis=-1).reshape(-1, 4)
            lin.append(g)
        lin = np.concatenate(lin).astype(np.uint32)
        _, _, _, d = engine.resolve(lin, subsample_snps=False, debug=True)
        want[r0:r0 + step] = d["cmats"].reshape(-1, per, 3, 16, 16).sum(axis=1, dtype=np.uint64)
    assert want.max() < 2**32
    assert np.array_equal(dbg["cmats"], want.astype(np.uint32))


def test_table_follows_a_bootstrap_replicate(engine, oracle):
    from tetrad_amd import synth
    tmparr, tmpmap, sp, _ = synth.simulate_species(8, 3, 3000, seed=4, block=0.2)
    K = 8
    seqarr, _, spans = synth.make_c5_source(source=(tmparr, tmpmap))
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    _, _, _, d0 = engine.resolve_species(rows, debug=True)          # builds the table of the first replicate
    assert np.array_equal(d0["cmats"], pooled_factored(tmparr, sp, K, rows))
    engine.set_source(seqarr, spans)
    rng = np.random.default_rng(2)
    for rep in range(2):
        engine.bootstrap(rng.integers(0, spans.shape[0], spans.shape[0]), 10 + rep, 20 + rep)
        arr, _ = engine.get_data()
        rstat, rscor, flags, d = engine.resolve_species(rows, debug=True)
        cm = pooled_factored(arr, sp, K, rows)
        assert np.array_equal(d["cmats"], cm), f"replicate {rep}: stale species table"
        check_rows(rstat, rscor, flags, cm, oracle)


def test_device_call_equals_host_call_on_two_streams(engine):
    import torch
    from tetrad_amd import synth
    T, K = 60, 15
    tmparr, tmpmap = synth.simulate_tmparr(T, 6000, seed=8)
    rng = np.random.default_rng(3)
    sp = random_map(T, K, rng)
    engine.set_data(tmparr, tmpmap)
    engine.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    host = engine.resolve_species(rows)
    engine.set_option("batch", 500)                 # several scan batches per call
    try:
        dev = torch.device("cuda:0")
        dq = torch.from_numpy(rows.view(np.int32)).to(dev)
        Q = rows.shape[0]
        outs = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
        for s in streams:
            drs = torch.empty((Q, 2), dtype=torch.int32, device=dev)
            dsc = torch.empty((Q, 3), dtype=torch.float64, device=dev)
            dfl = torch.empty(Q, dtype=torch.uint8, device=dev)
            engine.resolve_species_dev(dq.data_ptr(), Q, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), s.cuda_stream)
            outs.append((drs, dsc, dfl))
        torch.cuda.synchronize()
    finally:
        engine.set_option("batch", 0)
    for drs, dsc, dfl in outs:
        assert np.array_equal(drs.cpu().numpy().view(np.uint32), host[0])
        assert np.array_equal(dsc.cpu().numpy(), host[1])
        assert np.array_equal(dfl.cpu().numpy(), host[2])


def test_refusals(engine):
    import torch
    from tetrad_amd import _lib, synth
    from tetrad_amd.engine import QuartetEngine
    tmparr, tmpmap = synth.simulate_tmparr(12, 1000, seed=1)
    rows = np.array([[0, 1, 2, 3]], np.uint32)
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        with pytest.raises(_lib.TetradHipError, match="no species map"):
            eng.resolve_species(rows)
        with pytest.raises(_lib.TetradHipError, match="K >= 4"):
            eng.set_species(np.array([0, 1, 2] * 4, np.int32), 3)
        with pytest.raises(_lib.TetradHipError, match="T=11"):
            eng.set_species(np.arange(11, dtype=np.int32) % 4, 4)
        with pytest.raises(_lib.TetradHipError, match="outside"):
            eng.set_species(np.arange(12, dtype=np.int32), 5)
        eng.set_species(np.arange(12, dtype=np.int32) % 6, 6)
        with pytest.raises(_lib.TetradHipError, match="species id >= K"):
            eng.resolve_species(np.array([[0, 1, 2, 6]], np.uint32))
        # the device call flags the row instead
        dev = torch.device("cuda:0")
        bad = np.array([[0, 1, 2, 3], [0, 1, 2, 6]], np.uint32)
        dq = torch.from_numpy(bad.view(np.int32)).to(dev)
        drs = torch.empty((2, 2), dtype=torch.int32, device=dev)
        dsc = torch.empty((2, 3), dtype=torch.float64, device=dev)
        dfl = torch.empty(2, dtype=torch.uint8, device=dev)
        eng.resolve_species_dev(dq.data_ptr(), 2, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr())
        torch.cuda.synchronize()
        fl = dfl.cpu().numpy()
        assert fl[0] & _lib.FLAG_BAD_INDEX == 0 and fl[1] & _lib.FLAG_BAD_INDEX
        assert drs.cpu().numpy()[1, 1] == 0
        # a new replicate with another T: the map no longer fits
        eng.set_data(tmparr[:10], tmpmap)
        with pytest.raises(_lib.TetradHipError, match="T=12"):
            eng.resolve_species(rows)
        # the range rule: S x 16 x 16 x 16 x 16 >= 2^32 at S = 65 536
        big = np.zeros((64, 65_536), np.uint8)
        eng.set_data(big, np.zeros(65_536, np.uint32))
        eng.set_species(np.arange(64, dtype=np.int32) // 16, 4)
        with pytest.raises(_lib.TetradHipError, match="2\\^32"):
            eng.resolve_species(rows)
        # one lineage fewer per species is in range (65 536 x 15^4 < 2^32)
        eng.set_species(np.where(np.arange(64) % 16 == 15, -1, np.arange(64) // 16).astype(np.int32), 4)
        rstat, _, flags = eng.resolve_species(rows)
        assert rstat[0, 1] == 0 and flags[0] & _lib.FLAG_ZERO_DATA


def test_species_tree_end_to_end(engine):
    from tetrad_amd import qmc, species, synth
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.distributor import format_tsv_bytes
    K = 12
    tmparr, tmpmap, sp, true_nwk = synth.simulate_species(K, 3, 5000, seed=12)
    engine.set_data(tmparr, tmpmap)
    names = [f"sp{k:02d}" for k in range(K)]
    smap = species.SpeciesMap(sp, names)
    tree, (sq, rstat, rscor, flags) = species.infer_species_tree(engine, smap, return_rows=True)
    assert sq.shape == (495, 4)
    true_splits, _ = parse_tips_newick(true_nwk)
    num = tree
    for k in reversed(range(K)):
        num = num.replace(names[k], str(k))
    got_splits, tips = parse_tips_newick(num)
    assert tips == frozenset(range(K))
    assert true_splits <= got_splits
    # the rows are ordinary rows over K taxa: TSV, wQMC splits and concordance take them as they are
    assert format_tsv_bytes(sq, rscor, rstat).count(b"\n") == 495
    splits, _ = qmc.qmc_splits(sq, rscor, rstat)
    assert splits.shape[0] == 495
    want = np.array([quartet_topology(true_splits, q) for q in sq])
    assert np.all(flags == 0) and np.array_equal(rstat[:, 0], want)
    conc = Concordance(tree, samples=names)
    conc.add(sq, rscor, rstat, flags)
    st = conc.stats()
    induced = st["conc"] + st["disc1"] + st["disc2"]
    assert np.all(induced > 0)
    assert np.all(st["QC"] == 1.0)
