"""CPU: the host execution of the site concordance accumulator (`tq_scf_add`) against the
Python-integer model of tests/scf_model.py, every word bit for bit: all C(T,4) rows on small trees of every shape, rows
aimed at every edge at the sizes where the device kernel changes form and at the table limit; the row-order rule, the
refusals, `stats()`, `sample_edge_quartets` and `to_newick`."""
from itertools import combinations, permutations

import numpy as np
import pytest

from concordance_model import random_tree
from concordance_split_model import caterpillar, classify, collapse_clade, split_masks
from scf_model import (FX_CONC, FX_D1, FX_D2, NQ, NQ_ZERO, SUM_CONC, SUM_D1, SUM_D2, U32, ScfModel, assert_matches,
                       class_rows, scf_rows)
from tetrad_amd import _lib

K_TARGET = 4


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def make_tree(T, shape, rng):
    if shape == "binary":
        return random_tree(T, rng)
    if shape == "multifurcating":
        return random_tree(T, rng, multifurcate=0.3, rooted=False)
    if shape == "caterpillar":
        return caterpillar(T)
    assert shape == "polytomy"
    return collapse_clade(random_tree(T, rng, multifurcate=0.05), T, share=0.3)


def check_every_edge(acc, model, got):
    """Every edge received at least K_TARGET rows with a decisive site, in the model and in the library."""
    assert all(w[NQ] >= K_TARGET for w in model.words)
    assert (acc.raw()["edge_counts"][:, NQ] >= K_TARGET).all()
    assert all(w[NQ] >= K_TARGET for w in got)


@pytest.mark.parametrize("shape", ["binary", "multifurcating", "caterpillar", "polytomy"])
@pytest.mark.parametrize("T", [9, 13, 40])
def test_host_equals_model_all_quartets(T, shape):
    """All C(T,4) sets, positions shuffled, plus rows aimed at every edge and mixed rows with bad taxa."""
    from tetrad_amd.scf import SiteConcordance
    rng = np.random.default_rng([T, len(shape), 1])
    parent = make_tree(T, shape, rng)
    acc = SiteConcordance(parent, ntaxa=T)
    model = ScfModel(parent, T)
    if shape in ("binary", "caterpillar"):
        assert acc.n_edges == T - 3
    every = np.array(list(combinations(range(T), 4)), np.uint32)
    every = rng.permuted(every, axis=1)
    for sets, classes in ((every, class_rows(len(every), rng)), scf_rows(model, K_TARGET, 2000, rng)):
        acc.add(sets, classes)
        model.add(sets, classes)
    idx, got = assert_matches(acc, model)
    assert sorted(idx.tolist()) == list(range(acc.n_edges))
    check_every_edge(acc, model, got)
    assert model.skipped > 0 and any(w[NQ_ZERO] for w in model.words)


@pytest.mark.parametrize("shape", ["binary", "multifurcating", "caterpillar", "polytomy"])
@pytest.mark.parametrize("T", [129, 257, 2052, 4096])
def test_host_equals_model_large(T, shape):
    from tetrad_amd.scf import SiteConcordance
    rng = np.random.default_rng([T, len(shape), 2])
    parent = make_tree(T, shape, rng)
    acc = SiteConcordance(parent, ntaxa=T)
    model = ScfModel(parent, T)
    if shape in ("binary", "caterpillar"):
        assert acc.n_edges == T - 3
    n = 20_000 if T <= 257 else 6_000
    sets, classes = scf_rows(model, K_TARGET, n, rng, window=8 if shape == "caterpillar" else None)
    acc.add(sets, classes)
    model.add(sets, classes)
    idx, got = assert_matches(acc, model)
    assert sorted(idx.tolist()) == list(range(acc.n_edges))
    check_every_edge(acc, model, got)
    assert model.skipped > 0
    # reset, then the aimed rows alone
    acc.reset()
    m = K_TARGET * model.E
    acc.add(sets[:m], classes[:m])
    raw = acc.raw()
    assert (raw["edge_counts"][:, NQ] == K_TARGET).all() and raw["skipped"] == 0 and not raw["edge_counts"][:, NQ_ZERO].any()


def test_extreme_counts_by_hand():
    """(((0,1),4),(2,3)): the words of single rows, worked out here."""
    from tetrad_amd.scf import SiteConcordance
    parent = np.array([5, 5, 6, 6, 7, 7, 8, 8, -1], np.int32)       # (((0,1),4),(2,3)): edges {0,1} and {2,3}
    T = 5
    acc = SiteConcordance(parent, ntaxa=T)
    assert acc.n_edges == 2
    e01 = int(np.flatnonzero([set(np.flatnonzero(m)) in ({0, 1}, {2, 3, 4}) for m in acc.split_masks()])[0])

    def one(sets, n0, n1, n2):
        acc.reset()
        c = np.zeros((1, 16), np.uint32)
        c[0, [3, 6, 8]] = n0, n1, n2
        c[0, 15] = 77
        acc.add(np.array([sets], np.uint32), c)
        r = acc.raw()
        return [int(x) for x in r["edge_counts"][e01]], r["skipped"]

    full = (U32 << 32) // (3 * U32)
    assert one([0, 1, 2, 4], U32, U32, U32) == ([1, 0, U32, U32, U32, full, full, full], 0)
    assert full == (1 << 32) // 3
    assert one([0, 1, 2, 4], U32, 0, 0) == ([1, 0, U32, 0, 0, 1 << 32, 0, 0], 0)
    assert one([0, 1, 2, 4], 0, U32, U32) == ([1, 0, 0, U32, U32, 0, 1 << 31, 1 << 31], 0)
    assert one([0, 1, 2, 4], 0, 0, 0) == ([0, 1, 0, 0, 0, 0, 0, 0], 0)
    # r = 1: (0, 2, 1, 4) pairs position 0 with position 2; d1 is resolution 0, d2 resolution 2
    assert one([0, 2, 1, 4], 5, 7, 11) == ([1, 0, 7, 5, 11, (7 << 32) // 23, (5 << 32) // 23, (11 << 32) // 23], 0)
    # r = 2: d1 is resolution 0, d2 resolution 1
    assert one([0, 2, 4, 1], 5, 7, 11) == ([1, 0, 11, 5, 7, (11 << 32) // 23, (5 << 32) // 23, (7 << 32) // 23], 0)
    assert one([0, 1, 2, 2], 5, 7, 11) == ([0] * 8, 1)
    assert one([0, 1, 2, 5], 5, 7, 11) == ([0] * 8, 1)
    assert one([0, 1, 2, 0xFFFFFFFF], 5, 7, 11) == ([0] * 8, 1)
    # (0, 2, 3, 4) is induced on {2,3} only; (0, 1, 2, 3) on no edge: taxon 4 joins its internal path
    assert one([4, 0, 2, 1], 1, 2, 3)[0][NQ] == 1
    assert one([0, 2, 3, 4], 1, 2, 3) == ([0] * 8, 0) and int(acc.raw()["edge_counts"][1 - e01, NQ]) == 1
    assert one([0, 1, 2, 3], 1, 2, 3) == ([0] * 8, 0) and not acc.raw()["edge_counts"].any()


def test_row_order():
    """Permuting a row's positions and its class row with `permute_classes` leaves conc unchanged and moves d1 / d2
    as the rule says: by the index of the resolution in the permuted row."""
    from tetrad_amd.patterns import permute_classes
    from tetrad_amd.scf import SiteConcordance
    rng = np.random.default_rng(11)
    T = 12
    parent = random_tree(T, rng)
    acc = SiteConcordance(parent, ntaxa=T)
    masks = split_masks(parent, T)
    sets = np.array([q for q in combinations(range(T), 4)], np.int64)
    edge, res = classify(masks, sets)
    sets = sets[edge >= 0][:60]
    classes = class_rows(len(sets), rng, decisive=True)
    for q, c in zip(sets, classes):
        words = {}
        for perm in permutations(range(4)):
            pq = q[list(perm)]
            pc = permute_classes(c[None, :], perm)
            acc.reset()
            acc.add(pq.astype(np.uint32)[None, :], pc)
            e = np.flatnonzero(acc.raw()["edge_counts"][:, NQ])
            assert len(e) == 1
            w = [int(x) for x in acc.raw()["edge_counts"][e[0]]]
            # the rule, restated on the permuted row: r from the split, d1 = the lower other index
            _, r = classify(masks, pq[None, :])
            n = [int(pc[0, k]) for k in (3, 6, 8)]
            lower, other = [k for k in range(3) if k != r[0]]
            assert (w[SUM_CONC], w[SUM_D1], w[SUM_D2]) == (n[r[0]], n[lower], n[other])
            words[perm] = (int(e[0]), w)
        ref_e, ref = words[(0, 1, 2, 3)]
        for perm, (e, w) in words.items():
            assert e == ref_e and w[SUM_CONC] == ref[SUM_CONC] and w[FX_CONC] == ref[FX_CONC]
            assert sorted([w[SUM_D1], w[SUM_D2]]) == sorted([ref[SUM_D1], ref[SUM_D2]])
            assert sorted([w[FX_D1], w[FX_D2]]) == sorted([ref[FX_D1], ref[FX_D2]])


def test_refusals(lib):
    import ctypes
    from tetrad_amd.scf import SiteConcordance
    for T in (3, 4097):
        with pytest.raises(_lib.TetradHipError) as err:
            SiteConcordance(caterpillar(T), ntaxa=T)
        assert err.value.code == -1
    assert "limit of 4096 taxa" in str(err.value)
    assert SiteConcordance(caterpillar(4), ntaxa=4).n_edges == 1
    T = 9
    rng = np.random.default_rng(3)
    parent = random_tree(T, rng)
    acc = SiteConcordance(parent, ntaxa=T)
    sets = np.array(list(combinations(range(T), 4)), np.uint32)
    classes = class_rows(len(sets), rng)
    acc.add(sets, classes)
    before = acc.raw()
    # a device add without a context, NULL pointers, negative n: refused, the sums stay
    assert lib.tq_scf_add_dev(acc._h, sets.ctypes.data, classes.ctypes.data, len(sets), None) == -1
    assert b"without a context" in lib.tq_last_error(None)
    with pytest.raises(ValueError):
        acc.add_dev(None, None)
    assert lib.tq_scf_add(acc._h, None, classes.ctypes.data, 5) == -1
    assert lib.tq_scf_add(acc._h, sets.ctypes.data, None, 5) == -1
    assert lib.tq_scf_add(acc._h, sets.ctypes.data, classes.ctypes.data, -1) == -1
    assert b"tq_scf_add" in lib.tq_last_error(None)
    assert lib.tq_scf_add(acc._h, None, None, 0) == 0                 # n = 0 is valid
    assert lib.tq_scf_add(None, sets.ctypes.data, classes.ctypes.data, 1) == -1
    assert lib.tq_scf_read(None, None, None, None) == -1 and lib.tq_scf_reset(None) == -1
    assert lib.tq_scf_create(None, parent.ctypes.data, len(parent), T, None) == -1
    h = ctypes.c_void_p(123)
    assert lib.tq_scf_create(ctypes.byref(h), None, len(parent), T, None) == -1 and not h.value
    lib.tq_scf_destroy(None)
    with pytest.raises(ValueError):
        acc.add(sets, classes[:-1])
    after = acc.raw()
    np.testing.assert_array_equal(after["edge_counts"], before["edge_counts"])
    assert after["skipped"] == before["skipped"]
    assert lib.tq_scf_read(acc._h, None, None, None) == 0             # every output may be NULL


def test_stats():
    from tetrad_amd.scf import SiteConcordance
    rng = np.random.default_rng(8)
    T = 16
    parent = random_tree(T, rng)
    acc = SiteConcordance(parent, ntaxa=T)
    st = acc.stats()
    for k in ("sCF", "sDF1", "sDF2", "sN", "sCF_pooled", "sDF1_pooled", "sDF2_pooled"):
        assert st[k].shape == (T - 3,) and np.isnan(st[k]).all(), k
    assert not st["nq"].any() and not st["nq_zero"].any() and st["skipped"] == 0 and st["split"].shape == (T - 3, T)
    model = ScfModel(parent, T)
    sets, classes = scf_rows(model, K_TARGET, 5000, rng)
    # one edge gets rows without a decisive site only
    edge, _ = classify(model.masks, np.where(sets < T, sets, 0))
    classes[edge == 0] = 0
    acc.add(sets, classes)
    model.add(sets, classes)
    idx, got = assert_matches(acc, model)
    st = acc.stats()
    e0 = idx[0]
    assert st["nq"][e0] == 0 and st["nq_zero"][e0] >= K_TARGET
    for k in ("sCF", "sDF1", "sDF2", "sN", "sCF_pooled"):
        assert np.isnan(st[k][e0]), k
    rest = np.flatnonzero(np.arange(T - 3) != e0)
    total = st["sCF"][rest] + st["sDF1"][rest] + st["sDF2"][rest]
    assert (total <= 100.0 + 1e-12).all() and (100.0 - total <= 3 * 2.0**-32 * 100).all()
    for m, e in enumerate(idx):
        w = model.words[m]
        if not w[NQ]:
            continue
        assert st["sCF"][e] == pytest.approx(100 * w[FX_CONC] / (w[NQ] << 32), rel=1e-14)
        assert st["sDF1"][e] == pytest.approx(100 * w[FX_D1] / (w[NQ] << 32), rel=1e-14)
        assert st["sDF2"][e] == pytest.approx(100 * w[FX_D2] / (w[NQ] << 32), rel=1e-14)
        inf = w[SUM_CONC] + w[SUM_D1] + w[SUM_D2]
        assert st["sN"][e] == pytest.approx(inf / w[NQ], rel=1e-14)
        assert st["sCF_pooled"][e] == pytest.approx(100 * w[SUM_CONC] / inf, rel=1e-14)
        assert st["sDF1_pooled"][e] + st["sDF2_pooled"][e] == pytest.approx(100 * (w[SUM_D1] + w[SUM_D2]) / inf, rel=1e-13)


@pytest.mark.parametrize("shape", ["binary", "multifurcating", "caterpillar", "polytomy"])
def test_sample_edge_quartets(shape):
    from tetrad_amd.scf import sample_edge_quartets
    T = 60
    rng = np.random.default_rng([len(shape), 4])
    parent = make_tree(T, shape, rng)
    masks = split_masks(parent, T)
    rows = sample_edge_quartets(parent, T, 25, np.random.default_rng(77))
    assert rows.dtype == np.int64 and rows.ndim == 2 and rows.shape[1] == 4
    assert (rows[:, 1:] > rows[:, :-1]).all() and rows.min() >= 0 and rows.max() < T
    key = ((rows[:, 0] * T + rows[:, 1]) * T + rows[:, 2]) * T + rows[:, 3]
    assert (key[1:] > key[:-1]).all()                                   # strictly ascending, so unique
    assert len(rows) <= 25 * len(masks)
    edge, _ = classify(masks, rows)
    # every row is induced on an edge: on a polytomy two draws from one subtree off an end would not be
    assert (edge >= 0).all()
    assert np.array_equal(np.unique(edge), np.arange(len(masks)))       # every edge is hit
    again = sample_edge_quartets(parent, T, 25, np.random.default_rng(77))
    assert np.array_equal(rows, again)
    other = sample_edge_quartets(parent, T, 25, np.random.default_rng(78))
    assert other.shape != rows.shape or not np.array_equal(rows, other)
    assert sample_edge_quartets(parent, T, 0, np.random.default_rng(1)).shape == (0, 4)


def test_sample_edge_quartets_polytomy_ends_differ():
    """A star of four cherries around one node plus a clade: with few taxa per subtree a sampler that could draw both
    taxa of an end from one subtree would produce rows induced on no edge within a few draws."""
    from tetrad_amd.scf import sample_edge_quartets
    # root 14 with children: cherries (0,1) (2,3) (4,5) (6,7) and the tips 8, 9
    parent = np.array([10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 14, 14, 14, 14, -1], np.int32)
    T = 10
    masks = split_masks(parent, T)
    assert len(masks) == 4
    rows = sample_edge_quartets(parent, T, 200, np.random.default_rng(5))
    edge, _ = classify(masks, rows)
    assert (edge >= 0).all() and set(edge.tolist()) == {0, 1, 2, 3}
    # each row holds one whole cherry and two taxa from two other parts of the polytomy
    for q in rows:
        part = [int(parent[t]) if parent[t] != 14 else 100 + int(t) for t in q]
        assert sorted(np.bincount(np.unique(part, return_inverse=True)[1]).tolist()) == [1, 1, 2]


@pytest.mark.parametrize("rooted", [True, False])
def test_to_newick(rooted):
    import re
    from tetrad_amd.concordance import newick_to_parent
    from tetrad_amd.scf import SiteConcordance

    def text_of(parent, T):
        kids = {}
        for v, p in enumerate(parent):
            kids.setdefault(int(p), []).append(v)

        def w(v):
            return str(v) if v < T else "(" + ",".join(w(k) for k in kids[v]) + ")"
        return w(kids[-1][0]) + ";"

    rng = np.random.default_rng(21)
    T = 14
    parent = random_tree(T, rng, multifurcate=0.2, rooted=rooted)
    nwk = text_of(parent, T)
    acc = SiteConcordance(nwk)
    assert acc.T == T
    model = ScfModel(acc.parent, T)
    sets, classes = scf_rows(model, K_TARGET, 3000, rng)
    acc.add(sets, classes)
    out = acc.to_newick()
    assert out.endswith(";") and out.count("[&sCF=") == acc.n_edges
    par2, T2, names = newick_to_parent(out)
    assert T2 == T and names == [str(t) for t in range(T)]
    a = {m.tobytes() for m in split_masks(acc.parent, T)}
    b = {m.tobytes() for m in split_masks(par2, T)}
    assert a == b
    st = acc.stats()
    feats = re.findall(r"\[&sCF=([^,\]]+),sDF1=([^,\]]+),sDF2=([^,\]]+),sN=([^,\]]+),nq=(\d+)\]", out)
    assert len(feats) == acc.n_edges
    assert sorted(int(f[4]) for f in feats) == sorted(int(x) for x in st["nq"])
    assert sorted(f[0] for f in feats) == sorted("%.6g" % x for x in st["sCF"])
    # names through `samples`
    names = [f"t {i}" if i % 3 == 0 else f"s{i}" for i in range(T)]
    named = re.sub(r"(?<![\w])(\d+)(?![\w])", lambda m: "'%s'" % names[int(m.group(1))] if " " in names[int(m.group(1))]
                   else names[int(m.group(1))], nwk)
    acc2 = SiteConcordance(named, samples=names)
    acc2.add(sets, classes)
    np.testing.assert_array_equal(acc2.raw()["edge_counts"], acc.raw()["edge_counts"])
    out2 = acc2.to_newick()
    assert "'t 0'" in out2 and newick_to_parent(out2, names)[1] == T


def test_exports():
    import tetrad_amd
    from tetrad_amd import scf
    assert tetrad_amd.SiteConcordance is scf.SiteConcordance
    assert tetrad_amd.run_scf is scf.run_scf and tetrad_amd.sample_edge_quartets is scf.sample_edge_quartets
    for name in ("tq_scf_create", "tq_scf_destroy", "tq_scf_reset", "tq_scf_add", "tq_scf_add_dev", "tq_scf_shape",
                 "tq_scf_read"):
        assert name in _lib.SYMBOLS
