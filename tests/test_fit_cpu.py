"""CPU-only: the host execution of the quartet fit (`tq_stree_fit` on host rows) against the
independent split model of fit_model.py, and best-of-N builds on top of it (`Supertree.tree(restarts=N)`)."""
import ctypes

import numpy as np
import pytest

import fit_model as fm
from supertree_model import bad_rows, rows_from_tree, tree_children, tree_dist, true_topology
from tetrad_amd import _lib
from tetrad_amd.qmc import Supertree, infer_supertree_exact


@pytest.fixture(scope="module", autouse=True)
def built():
    _lib.build()


def candidates(children, root, T, seed):
    """name -> parent array: the generating tree, the star, a contraction, another tree; and three other writings of
    the generating tree (re-rooted, on a degree-2 root, with unary nodes) that must score as it does."""
    rng = np.random.default_rng(seed)
    gen = fm.parent_from_children(children, root, T)
    inner = [v for v in range(T, len(gen)) if gen[v] >= 0]
    other = fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(seed + 1000)), T)
    return {
        "generating": gen,
        "star": fm.star(T),
        "contracted": fm.contract(gen, T, rng),
        "other": other,
        "rerooted": fm.reroot(gen, inner[int(rng.integers(len(inner)))]),
        "deg2_root": fm.root_on_edge(gen, int(rng.integers(T))),
        "unary": fm.subdivide(gen, [int(v) for v in rng.choice(len(gen) - 1, size=min(5, T), replace=False)
                                    if gen[int(v)] >= 0]),
    }


def check_case(T, n, shape, wrong, weights, seed, scale=1.0, with_bad=False):
    children, root, q, sc, st = rows_from_tree(T, n, shape, wrong, seed)
    sc = sc * scale
    is_wrong = st[:, 0] != true_topology(tree_dist(children, root, T), q)
    fl = None
    if with_bad:
        rng = np.random.default_rng(seed)
        bq, bsc, bst, bfl = bad_rows(T, 70, rng)
        q, sc, st = np.concatenate([q, bq]), np.concatenate([sc, bsc]), np.concatenate([st, bst])
        fl = np.concatenate([np.zeros(n, np.uint8), bfl])
        perm = rng.permutation(len(q))
        q, sc, st, fl = q[perm], sc[perm], st[perm], fl[perm]
    cand = candidates(children, root, T, seed)
    names = list(cand)
    with Supertree(T, len(q), weights, min_snps=2 if with_bad else 0) as acc:
        acc.add(q, sc, st, fl)
        kept, skipped, sum_k = acc.counts()
        sp, k = acc.rows()
        res = acc.fit([cand[nm] for nm in names])
        assert len(res) == len(names)
        got = {nm: fm.as_ints(r) for nm, r in zip(names, res)}
        for nm in names:
            assert got[nm] == fm.model_fit(cand[nm], T, sp, k), nm
            assert sum(got[nm][:3]) == sum_k and sum(got[nm][3:]) == kept, nm
        for nm in ("rerooted", "deg2_root", "unary"):
            assert got[nm] == got["generating"], nm
        assert got["star"] == [0, 0, sum_k, 0, 0, kept]
        assert got["generating"][2] == 0 and got["generating"][5] == 0        # a binary tree resolves every quartet
        assert got["contracted"][0] <= got["generating"][0] and got["contracted"][1] <= got["generating"][1]
        if with_bad:
            assert skipped >= 50 and kept + skipped == len(q)
        else:
            assert kept == n and skipped == 0                               # so k is aligned with the rows as made
            assert got["generating"][1] == sum(int(x) for x in k[is_wrong])
            assert got["generating"][4] == int(is_wrong.sum())
            if wrong == 0.0:
                assert got["generating"][1] == 0
        if T >= 16 and wrong > 0:                                           # the mixed cases exercise every class
            for nm in ("contracted",):
                assert all(x > 0 for x in got[nm]), (nm, got[nm])
        # a single tree, and its fraction
        one = acc.fit(cand["other"])
        assert fm.as_ints(one) == got["other"]
        den = got["other"][0] + got["other"][1]
        assert one["fraction"] == got["other"][0] / den if den else np.isnan(one["fraction"])
        return k


@pytest.mark.parametrize("shape", ["random", "balanced", "caterpillar"])
@pytest.mark.parametrize("wrong", [0.0, 0.1, 0.4])
@pytest.mark.parametrize("T", [4, 5, 7, 16, 40])
def test_fit_equals_the_split_model(T, shape, wrong):
    weights = (T + int(wrong * 10)) % 4
    check_case(T, 600 if T >= 16 else 120, shape, wrong, weights, seed=T + len(shape))


@pytest.mark.parametrize("weights", [0, 1, 2, 3])
def test_every_weight_strategy_and_bad_rows_mixed_in(weights):
    check_case(23, 500, "random", 0.1, weights, seed=weights)
    check_case(23, 500, "random", 0.4, weights, seed=10 + weights, with_bad=True)


def test_weights_past_32_bits_sum_exactly():
    """strategy 1 with scores near 5e4: k near 5e9 >= 2^32, the sums far past 2^32"""
    k = check_case(40, 800, "random", 0.4, 1, seed=3, scale=1280.0)
    assert int(k.max()) >= 2**32 and int(k.sum(dtype=np.uint64)) > 2**40


def test_newick_input_and_names():
    T = 6
    _, _, q, sc, st = rows_from_tree(T, 200, "balanced", 0.2, 5)
    names = [f"s{i}" for i in range(T)]
    with Supertree(T, 200, 1) as acc:
        acc.add(q, sc, st)
        sp, k = acc.rows()
        nwk = "((0,1),(2,3),(4,5));"
        named = "((s0,s1),(s2,s3),(s4,s5));"
        par = np.array([6, 6, 7, 7, 8, 8, 9, 9, 9, -1], np.int32)
        want = fm.model_fit(par, T, sp, k)
        assert fm.as_ints(acc.fit(nwk)) == want
        assert fm.as_ints(acc.fit(named, samples=names)) == want
        both = acc.fit([nwk, "(0,1,2,3,4,5);"])
        assert fm.as_ints(both[0]) == want and fm.as_ints(both[1])[:2] == [0, 0]
        assert np.isnan(both[1]["fraction"])
        with pytest.raises(ValueError, match="tree 1"):
            acc.fit([nwk, "((0,1),(2,3),(4,4));"])
        with pytest.raises(ValueError, match="tree 0"):
            acc.fit(["((0,1),(2,3),4);"])


def raw_fit(acc, parents, n_nodes, out):
    lib = _lib.load()
    return lib.tq_stree_fit(acc._h, parents.ctypes.data, n_nodes.ctypes.data, len(n_nodes), parents.shape[1], None,
                            out.ctypes.data)


def test_a_bad_tree_refuses_the_whole_call():
    T = 10
    children, root, q, sc, st = rows_from_tree(T, 300, "random", 0.2, 8)
    good = fm.parent_from_children(children, root, T)
    missing = np.append(good, good[3])                      # a second tip beside taxon 3 that is no taxon
    cycle = np.append(good, [len(good) + 1, len(good)])     # two nodes that are each other's parent
    taken = good.copy()
    taken[4] = 5                                            # taxon 4 hangs below taxon 5
    lib = _lib.load()
    with Supertree(T, 300, 1) as acc:
        acc.add(q, sc, st)
        for bad, what in ((missing, "no children"), (cycle, "cycle"), (taken, "has children")):
            stride = len(good) + 2
            parents = np.full((4, stride), -1, np.int32)
            n_nodes = np.zeros(4, np.int64)
            for i, p in enumerate((good, good, bad, good)):
                parents[i, :len(p)] = p
                n_nodes[i] = len(p)
            out = np.full((4, 6), 12345, np.uint64)
            assert raw_fit(acc, parents, n_nodes, out) == -1
            msg = lib.tq_last_error(None).decode()
            assert "tree 2" in msg and what in msg, msg
            assert (out == 12345).all()
            with pytest.raises(_lib.TetradHipError, match="tree 2"):
                acc.fit([good, good, bad, good])
        # n_nodes past the stride
        parents = np.stack([good, good])
        out = np.full((2, 6), 7, np.uint64)
        assert raw_fit(acc, parents, np.array([len(good), len(good) + 1], np.int64), out) == -1
        assert "tree 1" in lib.tq_last_error(None).decode() and (out == 7).all()
        assert fm.as_ints(acc.fit(good)) == fm.model_fit(good, T, *acc.rows())      # still usable


def test_no_trees_and_no_rows_are_valid():
    T = 8
    children, root, q, sc, st = rows_from_tree(T, 100, "random", 0.0, 2)
    gen = fm.parent_from_children(children, root, T)
    lib = _lib.load()
    with Supertree(T, 100, 0) as acc:
        assert fm.as_ints(acc.fit(gen)) == [0] * 6                          # nothing added yet
        assert np.isnan(acc.fit(gen)["fraction"])
        assert lib.tq_stree_fit(acc._h, None, None, 0, 0, None, None) == 0  # R = 0
        assert len(acc.fit([])) == 0
        acc.add(q, sc, st)
        first = fm.as_ints(acc.fit(gen))
        assert first[1] == 0 and first[0] > 0
        acc.tree(3)                                                         # fits and builds alternate
        assert fm.as_ints(acc.fit(gen)) == first
        acc.reset()
        assert fm.as_ints(acc.fit(gen)) == [0] * 6


def test_a_sum_of_k_past_64_bits_is_refused():
    """strategy 1 weights near 4e9 give k near 4e14: 50 000 rows pass 2^64; the graph call reports 2^64 - 1"""
    T, n = 8, 50_000
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.0, 4)
    sc = np.full((n, 3), 3.9e9)
    with Supertree(T, n, 1) as acc:
        acc.add(q, sc, st)
        assert acc.counts()[2] == 2**64 - 1
        with pytest.raises(_lib.TetradHipError, match="64 bits"):
            acc.fit(fm.star(T))


@pytest.fixture(scope="module")
def noisy40():
    T, n = 40, 4000
    return (T, n) + rows_from_tree(T, n, "random", 0.4, seed=40)[2:]


def test_one_restart_is_todays_call(noisy40):
    T, n, q, sc, st = noisy40
    with Supertree(T, n, 1) as acc:
        acc.add(q, sc, st)
        for seed in (0, 7):
            assert acc.tree(seed, restarts=1) == acc.tree(seed)
        assert acc.last_fit is None
    assert infer_supertree_exact(q, sc, st, T, weights=1, seed=7, restarts=1) == \
        infer_supertree_exact(q, sc, st, T, weights=1, seed=7)


@pytest.mark.parametrize("search", ["f64", "exact"])
def test_best_of_eight(noisy40, search):
    T, n, q, sc, st = noisy40
    with Supertree(T, n, 1, search=search) as acc:
        acc.add(q, sc, st)
        seed = 11
        singles = [acc.tree(seed + i) for i in range(8)]
        stats = [(acc.tree(seed + i), acc.levels, acc.level_stats()[:, :3].copy()) for i in range(8)]
        fits = acc.fit(singles)
        best = acc.tree(seed, restarts=8)
        lf = acc.last_fit
        assert lf.seeds == [seed + i for i in range(8)] and len(lf.results) == 8
        np.testing.assert_array_equal(lf.results, fits)
        key = [(-int(r["k_satisfied"]), int(r["k_violated"]), i) for i, r in enumerate(fits)]
        assert lf.chosen == key.index(min(key))
        assert best == singles[lf.chosen]
        assert all(int(lf.results[lf.chosen]["k_satisfied"]) >= int(r["k_satisfied"]) for r in fits)
        assert acc.levels == stats[lf.chosen][1]
        np.testing.assert_array_equal(acc.level_stats()[:, :3], stats[lf.chosen][2])
        assert infer_supertree_exact(q, sc, st, T, weights=1, seed=seed, search=search, restarts=8) == best
        assert acc.tree(seed + 1) == singles[1]                             # back to a single build
        np.testing.assert_array_equal(acc.level_stats()[:, :3], stats[1][2])
        with pytest.raises(ValueError):
            acc.tree(seed, restarts=0)


def test_restarts_need_the_device_supertree():
    from tetrad_amd.replicates import bootstrap_trees
    with pytest.raises(ValueError, match="restarts"):
        bootstrap_trees(None, np.zeros((4, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 1, supertree="host", restarts=2)
