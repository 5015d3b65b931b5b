"""CPU: the split-mask model (tests/concordance_split_model.py) against the enumerating model at T <= 40, then the host
accumulator of the C ABI against the split model at the sizes where the device kernel changes form (T = 129, 256,
257), where the global-table form starts a second edge pass (2 051 / 2 052) and at the table limit (4 096): rows aimed
at every edge plus random rows with bad rows, rounding ties and boundary scores."""
import numpy as np
import pytest

from concordance_model import ConcordanceModel, random_tree
from concordance_split_model import (SplitModel, assert_raw_matches, caterpillar, classify, collapse_clade, dress_rows,
                                     mixed_rows, split_masks, targeted_rows)
from test_concordance_cpu import random_rows
from tetrad_amd import _lib
from tetrad_amd import concordance as C

K_TARGET = 4


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def make_tree(T, shape, rng):
    if shape == "binary":
        return random_tree(T, rng)
    if shape == "multifurcating":
        return random_tree(T, rng, multifurcate=0.15, rooted=False)
    if shape == "caterpillar":
        return caterpillar(T)
    assert shape == "polytomy"
    return collapse_clade(random_tree(T, rng, multifurcate=0.05), T, share=0.3)


@pytest.mark.parametrize("seed", range(12))
def test_split_model_equals_enumerating_model(seed):
    """The trees and rows of test_host_accumulator_equals_model_random_trees."""
    rng = np.random.default_rng(seed)
    T = int(rng.integers(4, 41))
    parent = random_tree(T, rng, multifurcate=0.3 if seed % 2 else 0.0, rooted=bool(seed % 3))
    min_snps = int(rng.integers(0, 10))
    min_ratio = float(rng.choice([0.0, 1.0, 1.1, 1.5]))
    old = ConcordanceModel(parent, T, min_snps, min_ratio)
    new = SplitModel(parent, T, min_snps, min_ratio)
    for _ in range(2):
        q, sc, st, fl = random_rows(T, 1500, rng)
        old.add(q, sc, st, fl)
        new.add(q, sc, st, fl)
    a, b = old.result(), new.result()
    assert b["skipped"] == a["skipped"]
    assert b["QFc"].tolist() == a["QFc"] and b["QFd"].tolist() == a["QFd"]
    np.testing.assert_array_equal(b["QF"], np.array(a["QF"]))             # NaN where no informative row
    sides = [frozenset(int(t) for t in np.flatnonzero(m)) for m in b["masks"]]
    assert len(sides) == len(a["edges"]) and set(sides) == set(a["edges"])
    for e, side in enumerate(sides):
        m = a["edges"][side]
        for k in ("conc", "disc1", "disc2", "nu"):
            assert int(b[k][e]) == m[k], (k, side)
        assert b["nqrts"][e] == m["nqrts"] and b["nsnps_sum"][e] == m["nsnps_sum"]
        assert b["weight_sum"][e] == pytest.approx(m["weight_sum"], rel=1e-12, abs=0)
        assert b["score_sum"][e] == pytest.approx(m["score_sum"], rel=1e-12, abs=0)
    if T >= 8:
        assert new.rows_induced > 0


def test_collapse_clade_makes_one_large_polytomy():
    rng = np.random.default_rng(1)
    T = 300
    parent = collapse_clade(random_tree(T, rng), T, share=0.3)
    deg = np.bincount(parent[parent >= 0])
    assert 60 <= deg.max() <= 120 and (deg[:T] == 0).all() and (deg[T:] >= 1).all()
    assert (parent == -1).sum() == 1
    assert len(split_masks(parent, T)) < T - 3 - 50


@pytest.mark.parametrize("shape", ["binary", "multifurcating", "caterpillar", "polytomy"])
@pytest.mark.parametrize("T", [129, 256, 257, 2051, 2052, 4096])
def test_host_accumulator_equals_split_model(T, shape):
    rng = np.random.default_rng([T, len(shape)])
    parent = make_tree(T, shape, rng)
    acc = C.Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25)
    model = SplitModel(parent, T, 3, 1.25)
    if shape in ("binary", "caterpillar"):
        assert acc.n_edges == T - 3
    tq, target = targeted_rows(model.masks, T, K_TARGET, rng, family=model.family)
    assert np.array_equal(np.bincount(target, minlength=model.E), np.full(model.E, K_TARGET))
    n = 20_000 if T <= 257 else 6_000
    for rows in (dress_rows(tq, rng), mixed_rows(T, n, rng, window=8 if shape == "caterpillar" else None)):
        acc.add(*rows)
        model.add(*rows)
    idx, raw, res = assert_raw_matches(acc, model)
    # the rows reached every edge, also in the library's own numbering
    assert (res["counted"] >= K_TARGET).all()
    assert (raw["edge_counts"][:, 1:5].sum(1) >= K_TARGET).all()
    assert sorted(idx.tolist()) == list(range(acc.n_edges))
    # a second add and a reset behave
    acc.reset()
    acc.add(*dress_rows(tq, np.random.default_rng(5)))
    assert (acc.raw()["edge_counts"][:, 1:5].sum(1) == K_TARGET).all() and acc.raw()["skipped"] == 0


def test_table_limit():
    T = 4096
    assert C.Concordance(caterpillar(T), ntaxa=T).n_edges == T - 3
    with pytest.raises(_lib.TetradHipError) as err:
        C.Concordance(caterpillar(T + 1), ntaxa=T + 1)
    assert err.value.code == -1 and "limit of 4096 taxa" in str(err.value)      # TQ_ERR_INVALID_ARG, as before
    # the model has no such limit: its classification of a row does not depend on a table size
    masks = split_masks(caterpillar(T + 1), T + 1)
    assert len(masks) == T - 2
    edge, res = classify(masks, np.array([[T, 3, T - 1, 2]]))
    assert edge[0] == -1
    edge, res = classify(masks, np.array([[T, 0, T - 1, 1]]))
    assert edge[0] == -1
    edge, res = classify(masks, np.array([[5, 7, 4, 6]]))
    assert edge[0] >= 0 and res[0] == 1                                  # (4, 5 | 6, 7): position 0 pairs with 2
