"""CPU: quartet concordance on a fixed tree (tetrad_amd.concordance, host accumulator of the C ABI) against the
pure-Python restatement in tests/concordance_model.py, which is itself pinned to the reference's functions through
tests/golden/concordance_fns.npz."""
import ctypes
from itertools import combinations

import numpy as np
import pytest

from concordance_model import ConcordanceModel, qc, qd, random_tree, row_values, row_values_reference, side_of
from conftest import GOLDEN, load_golden
from tetrad_amd import _lib
from tetrad_amd import concordance as C


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def random_rows(T, n, rng, bad=True):
    q = np.array([rng.choice(T, 4, replace=False) for _ in range(n)], np.uint32)   # unsorted positions
    sc = rng.uniform(0.0, 40.0, size=(n, 3))
    k = rng.random(n)
    sc[k < 0.1] = rng.integers(0, 40 * 128, size=(int((k < 0.1).sum()), 3)) / 128.0     # 6-decimal rounding ties
    sc[(k >= 0.1) & (k < 0.15)] = 0.0
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 30, n)], axis=1).astype(np.uint32)
    fl = np.zeros(n, np.uint8)
    if bad:
        m = rng.random(n)
        q[m < 0.02, 1] = q[m < 0.02, 0]                      # repeated taxon
        q[(m >= 0.02) & (m < 0.04), 2] = T                   # taxon >= T
        st[(m >= 0.04) & (m < 0.05), 0] = 3                  # topology > 2
        fl[(m >= 0.05) & (m < 0.10)] = rng.choice([1, 2, 4, 8, 16], size=int(((m >= 0.05) & (m < 0.10)).sum()))
    return q, sc, st, fl


def assert_matches_model(acc, model, rel=1e-12):
    s = acc.stats()
    res = model.result()
    assert s["skipped"] == res["skipped"]
    np.testing.assert_array_equal(s["QFc"], res["QFc"])
    np.testing.assert_array_equal(s["QFd"], res["QFd"])
    np.testing.assert_allclose(s["QF"], res["QF"], rtol=0, atol=0, equal_nan=True)
    assert len(res["edges"]) == acc.n_edges
    seen = set()
    for e in range(acc.n_edges):
        side = side_of(s["split"][e], acc.T)
        assert side in res["edges"] and side not in seen
        seen.add(side)
        m = res["edges"][side]
        for k in ("nqrts", "conc", "disc1", "disc2", "nu"):
            assert s[k][e] == m[k], (k, e)
        for k in ("QC", "QD"):
            assert s[k][e] == pytest.approx(m[k], rel=1e-15, abs=1e-15)
        for k in ("QI", "nsnps", "weights", "scores"):
            if np.isnan(m[k]):
                assert np.isnan(s[k][e])
            else:
                assert s[k][e] == pytest.approx(m[k], rel=rel, abs=0)


# -- the model against the reference's own functions -----------------------------------------------------------------
def test_model_and_library_qc_qd_equal_the_reference():
    g = load_golden("concordance_fns")
    for (a, b, c), rqc, rqd in zip(g["grid"], g["qc"], g["qd"]):
        assert qc(int(a), int(b), int(c)) == rqc and C.qc(int(a), int(b), int(c)) == rqc
        assert qd(int(b), int(c)) == rqd and C.qd(int(b), int(c)) == rqd


def test_row_values_pinned_to_the_reference_and_deviation_1():
    g = load_golden("concordance_fns")
    lines = g["tsv"].tobytes().decode().splitlines()
    np.testing.assert_array_equal(g["ref_quartets"], g["quartets"])
    np.testing.assert_array_equal(g["ref_topo"], g["topo"])
    for i, line in enumerate(lines):
        texts = line.split("\t")[4:7]
        assert row_values_reference(texts) == tuple(g["ref_values"][i, 1:])        # the restatement is exact
        w, s = row_values(g["scores"][i])
        if i == 3:                                                                  # scores 850.2 / 1200.5 / 1300.1
            assert w == g["ref_values"][i, 1]
            assert g["ref_values"][i, 2] == pytest.approx(1.2645848, abs=1e-7)    # string sort
            assert s == pytest.approx(1.4705951, abs=1e-7)                         # numeric sort (deviation 1)
        elif len({len(t.split(".")[0]) for t in texts}) == 1:                      # same digit counts: no deviation
            assert (w, s) == tuple(g["ref_values"][i, 1:])
        else:
            assert w == g["ref_values"][i, 1]


# -- newick --------------------------------------------------------------------------------------------------------
def test_newick_rooted_unrooted_names_quotes_lengths_supports():
    a = C.Concordance("((0,1),((2,3),(4,5)));")
    b = C.Concordance("(0,1,((2,3),(4,5)));")
    names = ["a", "b b", "c'd", "e", "f", "g"]
    c = C.Concordance("[&R] (( a:0.1 ,'b b':2e-3)90:1,((\"c'd\":1,e)0.5,(f[&x=1],g):3)[c]);".replace("\"c'd\"", "'c''d'"),
                      samples=names)
    ref = sorted(map(tuple, a.stats()["split"].astype(int).tolist()))
    assert sorted(map(tuple, b.stats()["split"].astype(int).tolist())) == ref
    assert sorted(map(tuple, c.stats()["split"].astype(int).tolist())) == ref
    assert a.n_edges == 3
    assert c.names == names


@pytest.mark.parametrize("nwk, samples", [
    ("((0,1),(2,4));", None),                  # taxon 3 missing
    ("((0,1),(2,3),(4,4));", None),            # duplicate
    ("((0,1),(2,3),(4,x));", None),            # not a taxon number
    ("((a,b),(c,d));", ["a", "b", "c", "d", "e"]),   # sample e missing
    ("((a,b),(c,z));", ["a", "b", "c", "d"]),   # extra name
    ("((0,1),2);", None),                      # T < 4
    ("((0,1),(2,3);", None),                   # unbalanced
])
def test_newick_refused(nwk, samples):
    with pytest.raises(ValueError):
        C.Concordance(nwk, samples=samples)


def test_bad_parent_arrays_are_error_codes(lib):
    h = ctypes.c_void_p()

    def create(par, T):
        par = np.asarray(par, np.int32)
        return lib.tq_conc_create(ctypes.byref(h), par.ctypes.data, par.shape[0], T, 0, 1.0, None)
    assert create([4, 4, 4, 4, -1], 4) == 0
    lib.tq_conc_destroy(h)
    assert create([4, 4, 4, -1, -1], 4) == -1          # two roots
    assert create([4, 4, 4, 4, 4], 4) == -1            # no root
    assert create([4, 4, 4, 4, 9], 4) == -1            # out of range
    assert create([5, 4, 4, 4, 5, 4, -1], 4) == -1     # cycle
    assert create([4, 4, 4, 4, -1, 4], 4) == -1        # a leaf that is no taxon
    assert create([3, 3, 3, -1], 3) == -1              # T < 4
    assert create([0, 4, 4, 4, -1], 4) == -1           # taxon with a child / self parent
    assert b"tq_conc_create" in lib.tq_last_error(None)
    assert lib.tq_conc_create(ctypes.byref(h), None, 5, 4, 0, 1.0, None) == -1
    assert lib.tq_conc_add(None, None, None, None, None, 0) == -1
    acc = C.Concordance("((0,1),(2,3),(4,5));")
    assert lib.tq_conc_add(acc._h, None, None, None, None, 3) == -1
    assert lib.tq_conc_add_dev(acc._h, None, None, None, None, 3, None) == -1     # no context: host-only
    with pytest.raises(ValueError):
        acc.add_dev(None, None, None)
    with pytest.raises(_lib.TetradHipError):
        C.Concordance(np.zeros(4097 * 2, np.int32), ntaxa=4097)                 # above the table limit


# -- host accumulator against the model ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_host_accumulator_equals_model_random_trees(seed):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(4, 41))
    parent = random_tree(T, rng, multifurcate=0.3 if seed % 2 else 0.0, rooted=bool(seed % 3))
    min_snps = int(rng.integers(0, 10))
    min_ratio = float(rng.choice([0.0, 1.0, 1.1, 1.5]))
    acc = C.Concordance(parent, ntaxa=T, min_snps=min_snps, min_ratio=min_ratio)
    model = ConcordanceModel(parent, T, min_snps, min_ratio)
    for _ in range(2):
        q, sc, st, fl = random_rows(T, 1500, rng)
        acc.add(q, sc, st, fl)
        model.add(q, sc, st, fl)
    assert_matches_model(acc, model)


def test_all_quartets_with_the_trees_own_topology():
    rng = np.random.default_rng(3)
    T = 12
    parent = random_tree(T, rng)
    model = ConcordanceModel(parent, T)
    q = np.array(list(combinations(range(T), 4)), np.uint32)
    perm = np.array([rng.permutation(4) for _ in range(len(q))])
    q = np.take_along_axis(q, perm, axis=1)                       # unsorted positions
    topo = np.zeros(len(q), np.uint32)
    for i, row in enumerate(q):
        hit = model.table.get(tuple(sorted(row.tolist())))
        if hit is not None:
            pairs = [frozenset((row[0], row[1])), frozenset((row[0], row[2])), frozenset((row[0], row[3]))]
            topo[i] = next(k for k in range(3) if pairs[k] in hit[1])
    sc = np.tile([1.0, 5.0, 5.0], (len(q), 1))
    st = np.stack([topo, np.full(len(q), 10, np.uint32)], axis=1)
    acc = C.Concordance(parent, ntaxa=T)
    acc.add(q, sc, st)
    model.add(q, sc, st)
    s = acc.stats()
    assert np.array_equal(s["conc"], s["nqrts"]) and (s["nqrts"] > 0).all()
    assert (s["QC"] == 1.0).all() and (s["QI"] == 1.0).all() and (s["QF"] == 1.0).all()
    assert_matches_model(acc, model)


def test_thresholds_at_their_boundaries():
    nwk = "((0,1),(2,3),(4,5));"
    par, T, _ = C.newick_to_parent(nwk)
    q = np.array([[0, 2, 4, 5]] * 6, np.uint32)
    sc = np.array([[1, 1.25, 1.25], [1, 1.25, 1.2499994], [1, 1.25, 1.2499996], [2, 2, 2], [0, 1, 1], [0, 0, 0]], float)
    st = np.array([[0, 5], [0, 5], [0, 4], [1, 5], [2, 5], [0, 0]], np.uint32)
    for min_snps, min_ratio in [(5, 1.25), (4, 1.25), (0, 1.0), (0, 0.0), (6, 0.0)]:
        acc = C.Concordance(nwk, min_snps=min_snps, min_ratio=min_ratio)
        model = ConcordanceModel(par, T, min_snps, min_ratio)
        acc.add(q, sc, st)
        model.add(q, sc, st)
        assert_matches_model(acc, model)
    acc = C.Concordance(nwk, min_snps=5, min_ratio=1.25)
    acc.add(q, sc, st)
    e = int(np.flatnonzero(acc.stats()["split"][:, 4])[0])
    # row 0: score exactly 1.25 -> informative; row 1: 1.2499994 reads back as 1.249999 -> uninformative;
    # row 2: 1.2499996 reads back as 1.25 but nsnps 4 < 5; rows 3-5: score 1, 0 (s0 == 0) and no data
    assert acc.stats()["conc"][e] == 1 and acc.stats()["nu"][e] == 5


def test_rounding_ties_read_back_like_the_tsv():
    from concordance_model import reread6
    xs = np.array([k / 128 for k in range(1, 4000, 2)] + [1e-7 * k + 0.5e-6 for k in range(200)] + [4294.9672955, 3e9 + 0.5e-6, 3999999999.9999995])
    xs = np.concatenate([xs, np.nextafter(xs, 0), np.nextafter(xs, np.inf)])
    # one edge, rows whose smallest score is x: score = weight / reread6(x)
    nwk = "((0,1),(2,3),(4,5));"
    acc = C.Concordance(nwk, min_ratio=0.0)
    q = np.tile(np.array([0, 1, 2, 4], np.uint32), (len(xs), 1))
    for i, x in enumerate(xs):
        acc.reset()
        acc.add(q[i:i + 1], np.array([[x, 4e9, 4e9]]), np.array([[0, 1]], np.uint32))
        s = acc.stats()
        e = int(np.argmax(s["conc"] + s["nu"]))
        y = reread6(x)
        assert s["scores"][e] == (4e9 / y if y else 0.0), x


# -- TSV path (deviation 3) and the supertree round trip -------------------------------------------------------------
def test_tsv_files_sum_like_one_accumulator(tmp_path):
    from tetrad_amd import distributor
    rng = np.random.default_rng(11)
    T = 14
    parent = random_tree(T, rng, multifurcate=0.2)
    acc_one = C.Concordance(parent, ntaxa=T, min_snps=2, min_ratio=1.05)
    model = ConcordanceModel(parent, T, 2, 1.05)
    files = []
    for k in range(3):
        q, sc, st, _ = random_rows(T, 700, rng, bad=False)
        q.sort(axis=1)
        p = tmp_path / f"quartets_{k}.tsv"
        p.write_text(distributor.format_tsv(q, sc, st))
        files.append(p)
        acc_one.add(q, sc, st)
        model.add(q, sc, st)
    nwk = tmp_path / "tree.nwk"
    names = [f"s{t}" for t in range(T)]
    acc_tmp = C.Concordance(parent, ntaxa=T)
    acc_tmp.names = names
    text = acc_tmp.to_newick()
    import re
    nwk.write_text(re.sub(r"\[&[^\]]*\]", "", text))
    got = C.run_quartet_concordance(nwk, files, min_snps=2, min_ratio=1.05, samples=names)
    a, b = got.stats(), acc_one.stats()
    order_a = [side_of(m, T) for m in a["split"]]
    order_b = [side_of(m, T) for m in b["split"]]
    idx = [order_b.index(x) for x in order_a]
    for k in ("nqrts", "conc", "disc1", "disc2", "nu"):
        np.testing.assert_array_equal(a[k], b[k][idx])
    for k in ("nsnps", "weights", "scores", "QC", "QD", "QI"):
        np.testing.assert_allclose(a[k], b[k][idx], rtol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(a["QFc"], b["QFc"])
    assert_matches_model(got, model)
    assert "[&QC=" in got.to_newick() and "s0[&QF=" in got.to_newick()


def test_to_newick_is_the_recorded_text():
    """The annotated newick of the tree and rows of `test_tsv_files_sum_like_one_accumulator`, one name quoted, byte for
    byte as tests/golden/concordance_newick_T14.txt records it (written by the recursive writer this one replaced)."""
    rng = np.random.default_rng(11)
    T = 14
    parent = random_tree(T, rng, multifurcate=0.2)
    acc = C.Concordance(parent, ntaxa=T, min_snps=2, min_ratio=1.05)
    for _ in range(3):
        q, sc, st, _ = random_rows(T, 700, rng, bad=False)
        q.sort(axis=1)
        acc.add(q, sc, st)
    acc.names = [f"s{t}" for t in range(T)]
    acc.names[3] = "s 3'x"
    assert acc.to_newick() + "\n" == (GOLDEN / "concordance_newick_T14.txt").read_text()


def test_to_newick_on_a_caterpillar_at_the_taxon_limit():
    """4 096 taxa in a caterpillar are 4 095 levels deep, past Python's recursion limit: the text is written without
    recursion, holds a comment for each of the T - 3 edges and each tip, and reads back as the same splits."""
    from concordance_split_model import caterpillar
    T = 4096
    acc = C.Concordance(caterpillar(T), ntaxa=T)
    q = np.array([[i, i + 1, i + 2, i + 3] for i in (0, 7, 2000, T - 4)], np.uint32)
    acc.add(q, np.tile([1.0, 2.0, 4.0], (4, 1)), np.tile(np.array([0, 9], np.uint32), (4, 1)))
    assert acc.raw()["edge_counts"][:, 1:5].sum() == 4
    text = acc.to_newick()
    assert text.count("[&QC=") == T - 3 and text.count("[&QF=") == T
    par, T2, _ = C.newick_to_parent(text)
    back = C.Concordance(par, ntaxa=T2)

    def sides(a):
        m = a.split_masks()
        return {np.packbits(r).tobytes() for r in np.where(m[:, :1], ~m, m)}

    assert T2 == T and back.n_edges == T - 3 and sides(back) == sides(acc)


def test_supertree_newick_goes_back_in():
    from tetrad_amd import qmc
    rng = np.random.default_rng(5)
    T = 10
    parent = random_tree(T, rng)
    model = ConcordanceModel(parent, T)
    splits = []
    for key, (side, (p1, p2)) in model.table.items():
        splits.append(sorted(p1) + sorted(p2))
    nwk = qmc.qmc_tree(np.array(splits, np.uint32), None, T)
    acc = C.Concordance(nwk)
    assert {side_of(m, T) for m in acc.stats()["split"]} == set(model.edges)
