"""GPU: the site concordance kernel (`tq_scf_add_dev`) equals the host execution and the
Python-integer model of tests/scf_model.py, every word bit for bit, at the sizes where `tree_acc_add_dev` changes form: the
last T of each LDS form and the first past it, the T whose binary tree fills exactly one tile of edges and one edge more,
and the table limit; at the row counts around the launcher's workgroup and grid boundaries; under every pattern of
adds; and end to end through `run_scf` against class rows counted from the raw matrix by tests/patterns_model.py."""
import ctypes
import functools
import re
from itertools import combinations

import numpy as np
import pytest

from conftest import load_golden
from concordance_model import random_tree
from concordance_split_model import caterpillar
from scf_model import NQ, ScfModel, assert_matches, class_rows, scf_rows

pytestmark = pytest.mark.gpu

# the constants of tetrad_amd/csrc/scf.hpp the sizes below come from (`test_constants` reads them from the source)
SCF_T_LDS_A = 128            # last T of the small LDS form
SCF_T_LDS_B = 256            # last T of the large LDS form; the global-table form starts at 257
SCF_EDGE_TILE = 2048         # edges per pass: a binary tree of T taxa has T - 3, so 2051 fills one pass
T_MAX = 4096                 # CONC_T_MAX
K_TARGET = 4

SIZES = [(5, "binary"), (SCF_T_LDS_A, "binary"), (SCF_T_LDS_A + 1, "binary"), (SCF_T_LDS_B, "binary"),
         (SCF_T_LDS_B + 1, "binary"), (SCF_EDGE_TILE + 3, "binary"), (SCF_EDGE_TILE + 4, "binary"), (T_MAX, "binary"),
         (T_MAX, "multifurcating"), (T_MAX, "caterpillar")]


def test_constants():
    from tetrad_amd import _lib
    text = (_lib.CSRC / "scf.hpp").read_text() + (_lib.CSRC / "concordance.hpp").read_text()
    for name, value in (("SCF_T_LDS_A", SCF_T_LDS_A), ("SCF_T_LDS_B", SCF_T_LDS_B), ("SCF_EDGE_TILE", SCF_EDGE_TILE),
                        ("CONC_T_MAX", T_MAX)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) == value, name


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


@functools.lru_cache(maxsize=None)
def case(T, shape):
    """(parent, sets, classes, model with the rows added): made once, shared, never changed."""
    rng = np.random.default_rng([T, len(shape), 19])
    if shape == "binary":
        parent = random_tree(T, rng)
    elif shape == "multifurcating":
        parent = random_tree(T, rng, multifurcate=0.15, rooted=False)
    else:
        parent = caterpillar(T)
    model = ScfModel(parent, T)
    n = 50_000 if T > SCF_T_LDS_B else 20_000
    sets, classes = scf_rows(model, K_TARGET, n, rng, window=8 if shape == "caterpillar" else None)
    model.add(sets, classes)
    for a in (parent, sets, classes):
        a.setflags(write=False)
    return parent, sets, classes, model


def to_dev(sets, classes):
    import torch
    return (torch.from_numpy(np.array(sets, np.uint32).view(np.int32)).cuda(),          # a copy: the shared rows are read-only
            torch.from_numpy(np.array(classes, np.uint32).view(np.int32)).cuda())


def assert_same(a, b):
    ra, rb = a.raw(), b.raw()
    np.testing.assert_array_equal(ra["edge_counts"], rb["edge_counts"])
    np.testing.assert_array_equal(ra["masks"], rb["masks"])
    assert ra["skipped"] == rb["skipped"]


@pytest.mark.parametrize("T,shape", SIZES)
def test_device_equals_host_equals_model(engine, T, shape):
    from tetrad_amd.scf import SiteConcordance
    parent, sets, classes, model = case(T, shape)
    if shape != "multifurcating":
        assert model.E == T - 3
    with SiteConcordance(parent, ntaxa=T, engine=engine) as dev, SiteConcordance(parent, ntaxa=T) as host:
        assert dev.n_edges == model.E
        dev.add_dev(*to_dev(sets, classes))
        host.add(sets, classes)
        assert_same(dev, host)
        idx, got = assert_matches(dev, model)
        assert sorted(idx.tolist()) == list(range(dev.n_edges))
        assert model.skipped > 0
        counts = dev.raw()["edge_counts"]
        assert (counts[:, NQ] >= K_TARGET).all()
        if model.E > SCF_EDGE_TILE:                      # the edges of the second pass, in the library's numbering
            assert len(counts[SCF_EDGE_TILE:]) == model.E - SCF_EDGE_TILE
            assert (counts[SCF_EDGE_TILE:, NQ] >= K_TARGET).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4097])
def test_row_counts(engine, n):
    """One row, one workgroup of rows and one more or less, one workgroup's share of the grid and one more."""
    from tetrad_amd.scf import SiteConcordance
    T = 40
    rng = np.random.default_rng([n, 3])
    parent = random_tree(T, rng, multifurcate=0.1)
    model = ScfModel(parent, T)
    sets, classes = scf_rows(model, 1, 5000, rng)
    sets, classes = sets[:n], classes[:n]
    model.add(sets, classes)
    with SiteConcordance(parent, ntaxa=T, engine=engine) as dev, SiteConcordance(parent, ntaxa=T) as host:
        dev.add_dev(*to_dev(sets, classes))
        host.add(sets, classes)
        assert_same(dev, host)
        assert_matches(dev, model)
        assert model.rows_induced > 0


def test_add_patterns(engine):
    import torch
    from tetrad_amd import _lib
    from tetrad_amd.scf import SiteConcordance
    T = SCF_T_LDS_B + 1
    parent, sets, classes, model = case(T, "binary")
    n = len(sets)
    d_sets, d_classes = to_dev(sets, classes)
    with SiteConcordance(parent, ntaxa=T, engine=engine) as one, SiteConcordance(parent, ntaxa=T, engine=engine) as two:
        one.add_dev(d_sets, d_classes)
        # two adds with other workgroup counts (3000 rows: one workgroup; the rest: several)
        h = 3000
        two.add_dev(d_sets[:h], d_classes[:h])
        two.add_dev(d_sets[h:], d_classes[h:])
        assert_same(one, two)
        assert_matches(two, model)
        # n = 0 changes nothing, with or without pointers
        two.add_dev(d_sets[:0], d_classes[:0])
        two.add_dev_ptrs(0, 0, 0)
        assert_same(one, two)
        # reset and repeat
        one.reset()
        assert not one.raw()["edge_counts"].any() and one.raw()["skipped"] == 0
        one.add_dev(d_sets, d_classes)
        assert_same(one, two)
        # two adds on two streams: ordered by the accumulator
        two.reset()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        two.add_dev(d_sets[:h], d_classes[:h], stream=s1)
        two.add_dev(d_sets[h:], d_classes[h:], stream=s2)
        assert_same(one, two)
        torch.cuda.synchronize()
        # host and device adds mixed into one read
        two.reset()
        two.add(sets[:h], classes[:h])
        two.add_dev(d_sets[h:], d_classes[h:])
        assert_same(one, two)
        assert_matches(two, model)
        # a misaligned pointer is refused and nothing is added
        before = two.raw()
        for ds, dc in ((d_sets.data_ptr() + 4, d_classes.data_ptr()), (d_sets.data_ptr(), d_classes.data_ptr() + 8)):
            with pytest.raises(_lib.TetradHipError) as err:
                two.add_dev_ptrs(ds, dc, 10)
            assert err.value.code == -1 and "16-byte aligned" in str(err.value)
        with pytest.raises(_lib.TetradHipError):
            two.add_dev_ptrs(d_sets.data_ptr(), d_classes.data_ptr(), -1)
        with pytest.raises(_lib.TetradHipError):
            two.add_dev_ptrs(0, d_classes.data_ptr(), 5)
        np.testing.assert_array_equal(two.raw()["edge_counts"], before["edge_counts"])
        assert two.raw()["skipped"] == before["skipped"]


def test_edge_order_is_that_of_the_concordance_accumulator(engine):
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.scf import SiteConcordance
    for T, shape in ((5, "binary"), (SCF_T_LDS_B + 1, "binary"), (T_MAX, "multifurcating")):
        parent = case(T, shape)[0]
        with SiteConcordance(parent, ntaxa=T, engine=engine) as s:
            c = Concordance(parent, ntaxa=T, engine=engine)
            np.testing.assert_array_equal(s.raw()["masks"], c.raw()["masks"])
            np.testing.assert_array_equal(s.split_masks(), c.split_masks())
            assert (s.n_edges, s.mask_words) == (c.n_edges, c.mask_words)
            c.close()


def test_both_accumulators_on_one_engine_across_streams(engine):
    """A `Concordance` and a `SiteConcordance` on one engine and one tree of T = 129 (the smallest on the 256-taxon LDS
    form), each with two device adds on two different streams, crosswise, equal their host adds word for word.  The
    concordance scores are integers whose smallest is 1, 2 or 4, so every weight is a multiple of 1/2, every score a
    multiple of 1/8, both at most 64: their f64 sums are exact in any order of addition, and the comparison is bitwise
    for those words too."""
    import torch
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.scf import SiteConcordance
    T = SCF_T_LDS_A + 1
    rng = np.random.default_rng([T, 23])
    parent = random_tree(T, rng)
    sets, classes = scf_rows(ScfModel(parent, T), 2, 128, rng)        # 2 rows aimed at every edge, 128 mixed rows
    n = len(sets)
    h = n // 3
    sc = np.stack([2.0 ** rng.integers(0, 3, n), rng.integers(4, 65, n), rng.integers(4, 65, n)], axis=1)
    sc = rng.permuted(sc.astype(np.float64), axis=1)
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 40, n)], axis=1).astype(np.uint32)
    d_sets, d_classes = to_dev(sets, classes)
    d_st, d_sc = torch.from_numpy(st.view(np.int32)).cuda(), torch.from_numpy(sc).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25, engine=engine) as cd, \
            Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25) as ch, \
            SiteConcordance(parent, ntaxa=T, engine=engine) as sd, SiteConcordance(parent, ntaxa=T) as sh:
        cd.add_dev(d_sets[:h], d_st[:h], d_sc[:h], None, stream=s1)
        sd.add_dev(d_sets[:h], d_classes[:h], stream=s2)
        cd.add_dev(d_sets[h:], d_st[h:], d_sc[h:], None, stream=s2)
        sd.add_dev(d_sets[h:], d_classes[h:], stream=s1)
        ch.add(sets, sc, st)
        sh.add(sets, classes)
        assert_same(sd, sh)
        got, want = cd.raw(), ch.raw()
        for k in ("edge_counts", "edge_sums", "masks", "tip_counts"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got["skipped"] == want["skipped"] == sh.raw()["skipped"] > 0
        assert (want["edge_counts"][:, 1:5].sum(axis=1) >= 2).all() and (want["edge_sums"] > 0).all()
        assert (sh.raw()["edge_counts"][:, NQ] >= 2).all()
        torch.cuda.synchronize()


# -- end to end ------------------------------------------------------------------------------------------------------
def model_of(parent, T, sets, classes):
    model = ScfModel(parent, T)
    model.add(sets, classes)
    return model


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("name", ["sparse_T10_S257", "c1_T16_S5000"])
def test_run_scf_goldens(engine, name, sub):
    import patterns_model as pm
    from tetrad_amd.scf import run_scf, sample_edge_quartets
    g = load_golden(name)
    tmparr, tmpmap = g["tmparr"], g["tmpmap"]
    T = tmparr.shape[0]
    parent = random_tree(T, np.random.default_rng([T, 5]))
    every = np.array(list(combinations(range(T), 4)), np.uint32)
    # all quartets, in chunks that do not divide their number
    stats, newick, acc = run_scf(engine, tmparr, tmpmap, parent, per_edge=None, subsample_snps=sub, chunk=500)
    model = model_of(parent, T, every, pm.model_classes(tmparr, tmpmap, every, sub))
    idx, got = assert_matches(acc, model)
    assert newick is None and stats["skipped"] == 0 and model.rows_induced > 0
    np.testing.assert_array_equal(stats["nq"][idx], [w[NQ] for w in model.words])
    acc.close()
    # the quartets around every branch
    stats, newick, acc = run_scf(engine, tmparr, tmpmap, parent, per_edge=10, subsample_snps=sub, seed=31)
    sets = sample_edge_quartets(parent, T, 10, np.random.default_rng(31))
    model = model_of(parent, T, sets, pm.model_classes(tmparr, tmpmap, sets, sub))
    assert_matches(acc, model)
    assert all(w[0] + w[1] >= 1 for w in model.words) and model.rows_induced == len(sets)
    acc.close()


def test_run_scf_newick_and_rng(engine):
    import patterns_model as pm
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.scf import run_scf, sample_edge_quartets
    g = load_golden("sparse_T10_S257")
    nwk = "((0,1),((2,(3,4)),(5,6)),(7,(8,9)));"
    parent = newick_to_parent(nwk)[0]
    stats, newick, acc = run_scf(engine, g["tmparr"], g["tmpmap"], nwk, per_edge=6, rng=np.random.default_rng(9))
    sets = sample_edge_quartets(parent, 10, 6, np.random.default_rng(9))
    assert_matches(acc, model_of(parent, 10, sets, pm.model_classes(g["tmparr"], g["tmpmap"], sets, False)))
    assert newick.count("[&sCF=") == acc.n_edges == 7
    acc.close()
    with pytest.raises(ValueError):
        run_scf(engine, g["tmparr"], g["tmpmap"], "((0,1),(2,3),4);")       # a tree of 5 taxa on 10 samples


def test_run_scf_species(engine):
    """A tree of species: the class rows are those of the pooled lineage counts (tests/species_model.py)."""
    import patterns_model as pm
    from species_model import lineage_data, pooled_factored
    from tetrad_amd.scf import run_scf
    sizes = [3, 1, 4, 2, 2, 1, 2]
    K = len(sizes)
    tmparr, tmpmap, sp = lineage_data(sizes, 900, seed=4, missing=0.1, p_within=0.15, left_out=1)
    parent = random_tree(K, np.random.default_rng(12))
    ssets = np.array(list(combinations(range(K), 4)), np.uint32)
    # the class of each of the 256 patterns 64 x0 + 16 x1 + 4 x2 + x3, from the model's own rule
    x = np.arange(256)
    table = pm.site_classes(np.stack([x >> 6, (x >> 4) & 3, (x >> 2) & 3, x & 3]).astype(np.uint8))
    want = pm.table_classes(pooled_factored(tmparr, sp, K, ssets)[:, 0].reshape(-1, 256), table)
    stats, _, acc = run_scf(engine, tmparr, tmpmap, parent, per_edge=None, species_of=sp, chunk=16)
    model = model_of(parent, K, ssets, want)
    assert_matches(acc, model)
    assert model.rows_induced > 0 and stats["skipped"] == 0
    acc.close()
    with pytest.raises(ValueError):
        run_scf(engine, tmparr, tmpmap, parent, subsample_snps=True, species_of=sp)
