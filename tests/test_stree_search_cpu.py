"""CPU: the exact integer cut search of the supertree (`stree_search_exact`).  The host execution
equals the plain-integer model of tests/stree_search_model.py on sides, cut flag and rounds; trees built under
`search="exact"` keep every promise of the exact supertree (tests/test_supertree_cpu.py) and recover what the f64 rule
recovers; `search="f64"` is the accumulator as it was."""
import ctypes
from itertools import combinations

import numpy as np
import pytest

import stree_search_model as model
from supertree_model import bipartitions, newick_bipartitions, rows_from_tree
from tetrad_amd import _lib, synth
from tetrad_amd.qmc import Supertree, infer_supertree_exact

SIZES = [4, 5, 8, 9, 63, 64, 65, 128, 129, 300]


@pytest.mark.parametrize("n", SIZES)
def test_host_search_equals_the_model(n):
    """tree graphs with 0 / 10 / 40 % wrong rows, all-zero B, all-zero G, tying cuts, the limit weights and their
    2^-20 copy; at n = 5 also a node whose first random start is refused"""
    cases = model.standard_cases([n])
    if n == 5:
        G, B = model.tree_graph(5, 40, 0.1, 55)
        cases.append(("forced", 5, G, B, model.forced_start_node(5)))
    want = model.model_batch(cases)
    got = model.run_batch(cases)
    for (name, _, G, B, _), w, g in zip(cases, want, got):
        assert g == (w[0], w[1], w[2]), name
    by_name = {c[0]: (c, w) for c, w in zip(cases, want)}
    assert not by_name["zeroB"][1][0] and by_name["zeroB"][1][2] == 0
    assert not by_name["zeroG"][1][0]                                       # good = 0 is no cut
    assert by_name["tree0"][1][0] and by_name["tie"][1][0]
    (_, _, G, B, _), (cut, side, _) = by_name["limit"]
    assert cut and int(B.sum()) // 2 == model.SUM_LIMIT - 1
    side = np.array(side)
    good, bad = model.cut_value(model.full(G, n), model.full(B, n), side)
    if n > 4:
        assert good * int(B.sum()) > 1 << 64                                # a cross product the rule may meet
    assert by_name["limit_small"][1][1] == by_name["limit"][1][1]           # the same sides at 2^-20 of the weights


def test_forced_start_exists_and_ties_tie():
    ns = model.forced_start_node(5)
    st0 = model.start_seed(ns, 0, 1)
    ones = sum(model.draw(st0, v) & 1 for v in range(5))
    assert ones < 2 or 5 - ones < 2
    # the tie graph at n = 4: splits k = 1 and k = 2 are worth the same, the first wins
    G, B = model.tie_graph(4)
    cut, side, rounds = model.search(G, B, 4, 1)
    assert cut and side == [0, 0, 1, 1] and rounds == 0
    assert not model.better((5, 3), (5, 3)) and model.better((5, 0), (4, 0)) and model.better((1, 0), (9, 1))


def test_the_draws_are_the_generators():
    """draw v of a start is the (v + 1)-th next() of QmcRng{start seed}"""
    st = model.start_seed(12345, 2, 7)
    state, outs = st, []
    for _ in range(5):
        state, o = model.rng_next(state)
        outs.append(o)
    assert outs == [model.draw(st, v) for v in range(5)]


@pytest.mark.parametrize("T,n,shape,wrong,weights", [(16, 1820, "random", 0.25, 1), (40, 40000, "caterpillar", 0.25, 2),
                                                     (128, 100000, "random", 0.1, 3), (60, 30000, "balanced", 0.4, 0)])
def test_exact_tree_is_independent_of_row_order_and_adds(T, n, shape, wrong, weights):
    rng = np.random.default_rng(T + n)
    _, _, q, sc, st = rows_from_tree(T, n, shape, wrong, seed=n)
    ref = infer_supertree_exact(q, sc, st, T, weights=weights, seed=3, search="exact")
    perm = rng.permutation(n)
    assert infer_supertree_exact(q[perm], sc[perm], st[perm], T, weights=weights, seed=3, search="exact") == ref
    for pieces in (1, 3, 17):
        with Supertree(T, n, weights, search="exact") as acc:
            for part in np.array_split(perm[::-1], pieces):
                acc.add(q[part], sc[part], st[part])
            assert acc.tree(3) == ref
            assert acc.tree(3) == ref                                       # build twice
            newick_bipartitions(acc.tree(4), T)                             # another seed may differ; still a tree


@pytest.mark.parametrize("T,seed", [(5, 1), (8, 2), (13, 3), (24, 4), (40, 5)])
def test_exact_recovers_the_generating_tree_from_all_its_quartets(T, seed):
    allq = np.array(list(combinations(range(T), 4)), np.uint32)
    children, root, q, sc, st = rows_from_tree(T, 0, "random", 0.0, seed, quartets=allq)
    truth = bipartitions(children, root, T)
    for s in (7, 8, 9):
        assert newick_bipartitions(infer_supertree_exact(q, sc, st, T, seed=s, search="exact"), T) == truth


@pytest.mark.parametrize("mode", ["sub", "full"])
@pytest.mark.parametrize("weights", [0, 1, 2, 3])
def test_exact_from_the_reference_rows_of_c1(mode, weights):
    """every split the f64 rule recovers there (all 13)"""
    from conftest import load_golden
    g = load_golden("c1_T16_S5000")
    children, root = synth.random_tree_children(16, np.random.default_rng(synth.CONFIG_SEEDS["c1"]))
    truth = bipartitions(children, root, 16)
    rows = (g["quartets"], g[f"{mode}_rscor"], g[f"{mode}_rstat"])
    f64 = newick_bipartitions(infer_supertree_exact(*rows, 16, weights=weights), 16)
    exact = newick_bipartitions(infer_supertree_exact(*rows, 16, weights=weights, search="exact"), 16)
    assert f64 & truth <= exact and exact == truth


def test_noisy_c5_shape_exact_against_f64():
    """T = 128, 400 000 sampled rows, 10 % wrong, seeds 0-4 on the same rows: the two rules draw different starts, so
    "exact" may recover one split fewer than "f64" per tree and no more.  Counts (f64 / exact of 125):
    125/125 at every seed."""
    T = 128
    children, root, q, sc, st = rows_from_tree(T, 400_000, "random", 0.1, seed=128)
    truth = bipartitions(children, root, T)
    assert len(truth) == 125
    with Supertree(T, len(q)) as acc:
        acc.add(q, sc, st)
        for seed in range(5):
            acc.set_search("f64")
            f64 = len(newick_bipartitions(acc.tree(seed), T) & truth)
            acc.set_search("exact")
            exact = len(newick_bipartitions(acc.tree(seed), T) & truth)
            print(f"seed {seed}: f64 {f64} exact {exact} of {len(truth)}")
            assert exact >= f64 - 1, (seed, f64, exact)


def test_f64_is_the_accumulator_as_it_was_and_switching_back():
    _, _, q, sc, st = rows_from_tree(40, 20000, "random", 0.4, seed=6)
    with Supertree(40, len(q), weights=1) as plain, Supertree(40, len(q), weights=1, search="f64") as named:
        plain.add(q, sc, st)
        named.add(q, sc, st)
        want = [plain.tree(s) for s in (0, 1, 2)]
        assert [named.tree(s) for s in (0, 1, 2)] == want
        named.set_search("exact")
        exact = [named.tree(s) for s in (0, 1, 2)]
        assert exact == [infer_supertree_exact(q, sc, st, 40, weights=1, seed=s, search="exact") for s in (0, 1, 2)]
        named.set_search("f64")
        assert [named.tree(s) for s in (0, 1, 2)] == want
        assert [infer_supertree_exact(q, sc, st, 40, weights=1, seed=s) for s in (0, 1, 2)] == want
        assert named.level_stats().shape[1] == 6


def test_invalid_rules_are_refused_and_a_valid_call_follows():
    lib = _lib.load()
    _, _, q, sc, st = rows_from_tree(16, 1500, "random", 0.1, seed=2)
    with pytest.raises(ValueError):
        Supertree(16, 10, search="integer")
    with pytest.raises(ValueError):
        infer_supertree_exact(q, sc, st, 16, search="")
    with Supertree(16, len(q), search="exact") as acc:
        acc.add(q, sc, st)
        ref = acc.tree(1)
        for bad in (-1, 2, 7):
            assert lib.tq_stree_set_search(acc._h, bad) == -1
        with pytest.raises(ValueError):
            acc.set_search("F64")
        assert acc.search == "exact" and acc.tree(1) == ref                 # the rule stayed
        assert lib.tq_stree_set_search(acc._h, 0) == 0
        assert acc.tree(1) == infer_supertree_exact(q, sc, st, 16, seed=1)
    assert lib.tq_stree_set_search(None, 1) == -1
    # the test hook refuses sizes outside its range and NULL pointers
    sizes = np.array([3], np.int32)
    z = np.zeros(8, np.uint64)
    out = np.zeros(8, np.uint8)
    assert lib.tq_stree_search(None, 1, sizes.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, out.ctypes.data,
                               out.ctypes.data, None) == -1
    assert lib.tq_stree_search(None, 1, None, z.ctypes.data, z.ctypes.data, z.ctypes.data, out.ctypes.data,
                               out.ctypes.data, None) == -1
    from tetrad_amd.replicates import bootstrap_trees
    with pytest.raises(ValueError, match="exact"):
        bootstrap_trees(None, np.zeros((4, 8), np.uint8), np.array([[0, 8]]), 1, 1, supertree="host", search="exact")
    with pytest.raises(ValueError):
        bootstrap_trees(None, np.zeros((4, 8), np.uint8), np.array([[0, 8]]), 1, 1, supertree="device", search="int")
