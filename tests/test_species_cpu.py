"""Species mode on the CPU: the pooling definition against its factored form, scores of pooled matrices, the imap
reader and the range rule."""
from itertools import combinations

import numpy as np
import pytest

from species_model import (flattenings, parse_tips_newick, pooled_factored, pooled_literal, quartet_topology,
                           score_rows, worker_mask)
from tetrad_amd import species, synth


def _case(seed, sizes, S, missing, block=0.0, left_out=1):
    rng = np.random.default_rng(seed)
    T = sum(sizes) + left_out
    tmparr, tmpmap = synth.simulate_radseq(T, S, seed, block=block, cell=missing) if block else \
        synth.simulate_tmparr(T, S, seed, missing=missing)
    species_of = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)] + [np.full(left_out, -1, np.int32)])
    species_of = rng.permutation(species_of)
    return tmparr, tmpmap, species_of


@pytest.mark.parametrize("seed,sizes,S,missing,block", [
    (1, (1, 2, 3, 4, 2), 300, 0.15, 0.0),
    (2, (6, 1, 2, 1, 5), 200, 0.10, 0.0),
    (3, (3, 3, 2, 4), 257, 0.02, 0.3),
    (4, (1, 1, 1, 1, 1, 1), 130, 0.0, 0.0),
])
def test_literal_equals_factored(oracle, seed, sizes, S, missing, block):
    tmparr, tmpmap, species_of = _case(seed, sizes, S, missing, block)
    K = len(sizes)
    rng = np.random.default_rng(seed + 7)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    # rows that repeat a species follow the definition literally
    rows = np.concatenate([rows, rng.integers(0, K, size=(3, 4)).astype(np.uint32)])
    lit = pooled_literal(oracle, tmparr, tmpmap, species_of, K, rows)
    fac = pooled_factored(tmparr, species_of, K, rows)
    assert np.array_equal(lit, fac)
    assert lit[:, 0].sum() > 0


def test_singletons_are_the_worker(oracle):
    """Each sample its own species: the pooled matrix is the worker's own count matrix."""
    tmparr, tmpmap = synth.simulate_tmparr(7, 400, 5)
    sp = np.arange(7, dtype=np.int32)
    rows = np.array(list(combinations(range(7), 4))[:20], np.uint32)
    _, _, _, dbg = oracle.new_infer_resolved_quartets(tmparr, tmpmap, rows, False, debug=True)
    assert np.array_equal(pooled_factored(tmparr, sp, 7, rows), dbg["cmats"])


def test_flattening_layout():
    t = np.arange(256, dtype=np.uint32).reshape(4, 4, 4, 4)
    f = flattenings(t)
    assert f[0, 4 * 1 + 2, 4 * 3 + 0] == t[1, 2, 3, 0]
    assert f[1, 4 * 1 + 3, 4 * 2 + 0] == t[1, 2, 3, 0]
    assert f[2, 4 * 1 + 0, 4 * 2 + 3] == t[1, 2, 3, 0]
    assert worker_mask(np.array([[0, 1], [0, 1], [0, 78], [0, 2]])).tolist() == [True, True]


def test_pooled_scores_find_the_species_tree(oracle):
    tmparr, tmpmap, species_of, nwk = synth.simulate_species(7, 3, 3000, seed=21)
    splits, tips = parse_tips_newick(nwk)
    assert tips == frozenset(range(7))
    rows = np.array(list(combinations(range(7), 4)), np.uint32)
    cm = pooled_factored(tmparr, species_of, 7, rows)
    rstat, _, zero = score_rows(oracle, cm)
    assert not zero.any()
    want = [quartet_topology(splits, q) for q in rows]
    assert [int(t) for t in rstat[:, 0]] == want


def test_simulate_species_shape_and_determinism():
    a = synth.simulate_species(5, 2, 500, seed=3, block=0.2)
    b = synth.simulate_species(5, 2, 500, seed=3, block=0.2)
    tmparr, tmpmap, species_of, nwk = a
    assert tmparr.shape == (10, 500) and tmpmap.shape == (500, 2)
    assert np.bincount(species_of).tolist() == [2] * 5
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert (tmparr == 78).mean() > 0.1
    assert np.all(np.diff(tmpmap[:, 0].astype(np.int64)) >= 0)


def test_read_imap_and_species_map(tmp_path):
    p = tmp_path / "imap.txt"
    p.write_text("# clade sample\nzeta z1\nalpha a1\nalpha a2\n\nmid m1\nbeta b1\n")
    imap = species.read_imap(p)
    assert imap == {"zeta": ["z1"], "alpha": ["a1", "a2"], "mid": ["m1"], "beta": ["b1"]}
    samples = ["a1", "b1", "x", "m1", "a2", "z1"]
    sm = species.SpeciesMap.from_imap(imap, samples)
    assert sm.names == ["alpha", "beta", "mid", "zeta"]
    assert sm.species_of.tolist() == [0, 1, -1, 2, 0, 3]
    assert sm.K == 4 and sm.sizes.tolist() == [2, 1, 1, 1]


def test_species_map_errors(tmp_path):
    bad = tmp_path / "bad.txt"
    bad.write_text("alpha a1 extra\n")
    with pytest.raises(ValueError, match="expected 'clade sample'"):
        species.read_imap(bad)
    samples = ["a", "b", "c", "d", "e"]
    with pytest.raises(ValueError, match="unknown sample"):
        species.SpeciesMap.from_imap({"A": ["a"], "B": ["b"], "C": ["c"], "D": ["q"]}, samples)
    with pytest.raises(ValueError, match="in two clades"):
        species.SpeciesMap.from_imap({"A": ["a"], "B": ["b", "a"], "C": ["c"], "D": ["d"]}, samples)
    with pytest.raises(ValueError, match="at least 4 clades"):
        species.SpeciesMap.from_imap({"A": ["a"], "B": ["b"], "C": ["c"]}, samples)


def test_range_rule():
    assert species.pooled_range_ok(50_000, [4] * 32)
    assert species.pooled_range_ok(2**32 // 16 - 1, [2, 2, 2, 2, 1])
    assert not species.pooled_range_ok(2**32 // 16, [2, 2, 2, 2, 1])
    assert not species.pooled_range_ok(10, [256, 1, 1, 1])
    # the edge the GPU tests run at: 11^4 x 293 352 = 4 294 966 632 < 2^32 = 4 294 967 296 <= 11^4 x 293 353
    assert species.pooled_range_ok(293_352, [11, 11, 11, 11])
    assert not species.pooled_range_ok(293_353, [11, 11, 11, 11])
    assert species.pooled_range_ok(1, [255, 255, 255, 255, 2, 1]) and not species.pooled_range_ok(2, [255] * 4)
    assert species.pooled_range_ok(20_000, [12, 13, 16, 17, 20]) and species.pooled_range_ok(200, [255, 100, 40, 17, 3, 1])
    assert not species.pooled_range_ok(10, [1, 1, 1])


def test_rows_with_bit_31_through_the_host_consumers(oracle):
    """The data of the GPU bit-31 test on the CPU: the model's figures, then rows with nsnps >= 2^31 through the TSV
    formatter and the host concordance accumulator (u64 nsnps sum)."""
    from species_model import spike_data
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.distributor import format_tsv_bytes
    tmparr, sp = spike_data(293_000)
    rows = np.array([[0, 1, 2, 3], [0, 2, 1, 3], [3, 2, 1, 0], [0, 0, 2, 2]], np.uint32)
    cm = pooled_factored(tmparr, sp, 4, rows)
    assert int(cm[0].max()) == 2_579_729_559 and int(cm[0, 0].sum(dtype=np.uint64)) == 4_263_722_738
    rstat, rscor, zero = score_rows(oracle, cm)
    assert not zero.any() and np.all(np.isfinite(rscor)) and int(rstat[0, 1]) == 4_263_722_738
    lines = format_tsv_bytes(rows, rscor, rstat).decode().splitlines()
    assert [ln.split("\t")[8] for ln in lines] == [str(int(n)) for n in rstat[:, 1]]
    assert lines[0].startswith("0\t1\t2\t3\t") and lines[0].endswith("\t4263722738")
    acc = Concordance("((0,1),2,(3,4));")
    acc.add(rows, rscor, rstat)
    r = acc.raw()
    assert r["skipped"] == 1 and int(r["edge_counts"][:, 1:5].sum()) == 3
    assert int(r["edge_counts"][:, 5].sum()) == sum(int(n) for n in rstat[:3, 1]) > 2**33


def test_lineage_data_counts():
    from species_model import lineage_data, species_counts
    sizes = (255, 100, 40, 17, 3, 1)
    tmparr, tmpmap, sp = lineage_data(sizes, 200, 31)
    assert tmparr.shape == (417, 200) and np.bincount(sp[sp >= 0]).tolist() == list(sizes)
    assert (species_counts(tmparr, sp, 6).max(axis=2) == np.array(sizes)[:, None]).all()
    noisy, _, sp2 = lineage_data(sizes, 200, 31, missing=0.2, p_within=0.02)
    assert np.array_equal(sp, sp2) and 0.15 < (noisy == 78).mean() < 0.25
    cnt = species_counts(noisy, sp, 6)
    assert cnt[0].max() > 150 and (cnt.sum(axis=2) <= np.array(sizes)[:, None]).all()


def test_species_quartets():
    assert species.species_quartets(6).shape == (15, 4)
    s = species.species_quartets(12, 40, seed=1)
    assert s.shape == (40, 4) and len({tuple(r) for r in s}) == 40
    assert np.all(np.diff(s, axis=1) > 0)
