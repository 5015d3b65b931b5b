"""CPU-only: the host back end of the consensus accumulator (`tq_cons_*` with a NULL context) and its Python layer
against the independent model of tests/consensus_model.py.  Every comparison is exact."""
import ctypes
import re

import numpy as np
import pytest

import consensus_model as cm
from tetrad_amd import _lib, qmc
from tetrad_amd.consensus import Consensus, consensus_tree, min_count_for, run_consensus


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def newick_of(parent, T):
    """Newick text of a parent array (numeric tips), children in node order."""
    kids = cm.kids_of(parent)
    root = [int(p) for p in parent].index(-1)
    text = {}
    order = [root]
    for v in order:
        order.extend(kids[v])
    for v in reversed(order):
        text[v] = str(v) if v < T else "(" + ",".join(text.pop(k) for k in kids[v]) + ")"
    return text[root] + ";"


def check(trees, T, freqs=(0.5, 0.3, 1.0, 0.0)):
    tab, n = cm.model_of(trees, T)
    with Consensus(T) as acc:
        acc.add_parents(trees)
        cm.assert_matches(acc, tab, n, T)
        for f in freqs:
            k = cm.min_count(f, n)
            assert min_count_for(f, n) == k
            assert acc.tree(f) == cm.consensus(tab, T, n, k), f
    return tab, n


@pytest.mark.parametrize("T", [4, 5, 6, 12, 33, 64, 65, 100])
def test_table_and_tree_match_the_model(T):
    check(cm.tree_set(T, seed=T), T)


def test_copies_of_one_tree():
    T, R = 20, 7
    t = cm.random_binary(T, np.random.default_rng(3))
    tab, n = check([t] * R, T)
    assert len(tab) == T - 3 and all(c == R for _, c in tab)
    with Consensus(T) as acc:
        acc.add_parents([t] * R)
        nwk = acc.tree()
    back = Consensus(T)
    back.add_newick([nwk])
    assert {s for s, _ in cm.table([cm.splits_of(t, T)])} == {frozenset(np.flatnonzero(m)) for m in back.splits()[0]}
    assert set(re.findall(r"\)(\d+)", nwk)) == {"100"}


@pytest.mark.parametrize("T", [4, 9])
def test_star_and_four_taxa_give_an_empty_table(T):
    with Consensus(T) as acc:
        acc.add_parents([cm.star(T)] * 3)
        masks, counts, n = acc.splits()
        assert masks.shape == (0, T) and len(counts) == 0 and n == 3
        assert acc.tree() == "(" + ",".join(str(t) for t in range(T)) + ");"
        assert acc.support_of(cm.star(T))[0].shape == (0,)


def test_the_one_split_of_four_taxa():
    with Consensus(4) as acc:
        acc.add_parents([cm.balanced(4), cm.unrooted(cm.balanced(4), 4), cm.star(4)])
        masks, counts, n = acc.splits()
        assert masks.tolist() == [[False, False, True, True]] and counts.tolist() == [2] and n == 3
        assert acc.tree() == "(0,1,(2,3)67);"


def quartet_tree(T, pair):
    """A tree of T taxa whose only split is `pair` (two taxa, neither taxon 0) against the rest."""
    parent = np.full(T + 2, T, np.int32)
    parent[T] = -1
    parent[T + 1] = T
    parent[list(pair)] = T + 1
    return parent


def test_half_and_half_conflict():
    T = 8
    A, B = quartet_tree(T, (1, 2)), quartet_tree(T, (2, 3))        # {1,2} and {2,3} overlap: incompatible
    with Consensus(T) as acc:
        acc.add_parents([A] * 5 + [B] * 5)
        assert acc.tree(0.5) == "(0,1,2,3,4,5,6,7);"               # 2 x 5 is not more than 10
        assert acc.tree(0.4) == "(0,(1,2)50,3,4,5,6,7);"           # {1,2} = 6 comes before {2,3} = 12
        assert acc.tree(0.4) == cm.consensus(cm.model_of([A] * 5 + [B] * 5, T)[0], T, 10, 4)


def test_three_way_conflict():
    T = 9
    A, B, C = quartet_tree(T, (1, 2)), quartet_tree(T, (2, 3)), quartet_tree(T, (1, 3))
    trees = [A] * 8 + [B] * 7 + [C] * 5                            # 40 / 35 / 25 percent
    tab, n = check(trees, T, freqs=(0.5, 0.4, 0.36, 0.35, 0.25, 0.1))
    with Consensus(T) as acc:
        acc.add_parents(trees)
        assert acc.tree(0.5) == "(0,1,2,3,4,5,6,7,8);"
        assert acc.tree(0.25) == "(0,(1,2)40,3,4,5,6,7,8);"
    with Consensus(T) as acc:                                      # the most frequent split wins whatever the mask order
        acc.add_parents([A] * 5 + [B] * 7 + [C] * 8)
        assert acc.tree(0.25) == "(0,(1,3)40,2,4,5,6,7,8);"


def test_min_count_boundary():
    T = 8
    A, B = quartet_tree(T, (1, 2)), quartet_tree(T, (4, 5))
    with Consensus(T) as acc:
        acc.add_parents([A] * 6 + [B] * 5 + [cm.star(T)] * 9)
        assert acc.tree_min_count(6) == "(0,(1,2)30,3,4,5,6,7);"   # count 6 = min_count is in, count 5 is out
        assert acc.tree_min_count(5) == "(0,(1,2)30,3,(4,5)25,6,7);"
        assert acc.tree_min_count(7) == "(0,1,2,3,4,5,6,7);"
    assert min_count_for(0.4, 5) == 2 and min_count_for(0.5, 10) == 6 and min_count_for(0.5, 9) == 5
    assert min_count_for(0.0, 7) == 1 and min_count_for(1.0, 7) == 7


def test_rooting_and_unary_nodes_do_not_matter():
    T = 17
    rng = np.random.default_rng(5)
    t = cm.random_binary(T, rng)
    tables = []
    for form in (t, cm.unrooted(t, T), cm.with_unary(t, T, rng, 5), cm.with_unary(cm.unrooted(t, T), T, rng, 2)):
        with Consensus(T) as acc:
            acc.add_parents([form])
            tables.append(acc.raw())
    for masks, counts, n in tables[1:]:
        np.testing.assert_array_equal(masks, tables[0][0])
        np.testing.assert_array_equal(counts, tables[0][1])


def test_several_adds_and_reset():
    T = 33
    trees = cm.tree_set(T, seed=9)
    with Consensus(T) as one, Consensus(T) as many:
        one.add_parents(trees)
        for i in range(0, len(trees), 7):
            many.add_parents(trees[i:i + 7])
        for a, b in zip(one.raw(), many.raw()):
            np.testing.assert_array_equal(a, b)
        first = many.raw()
        many.reset()
        assert many.ntrees == 0 and len(many.raw()[1]) == 0
        many.add_parents(trees)
        for a, b in zip(first, many.raw()):
            np.testing.assert_array_equal(a, b)


def test_map_supports_keeps_the_given_tree():
    T = 8
    A, B = quartet_tree(T, (1, 2)), quartet_tree(T, (4, 5))
    given = "((((1,2),3),0),((5,4),(6,7)));"                       # rooted, its own child order
    with Consensus(T) as acc:
        acc.add_parents([A] * 3 + [B] * 1)
        out = acc.map_supports(given)
        counts, masks = acc.support_of(given)
    # {1,2} 3 of 4, {1,2,3} never, {0,1,2,3} | {4,5,6,7} never (labelled once, on the first node in preorder), {4,5} 1 of 4
    assert out == "((((1,2)75,3)0,0)0,((5,4)25,(6,7)0));"
    want = {frozenset(s): c for s, c in [((1, 2), 3), ((1, 2, 3), 0), ((4, 5, 6, 7), 0), ((4, 5), 1), ((6, 7), 0)]}
    assert {frozenset(np.flatnonzero(m)): int(c) for m, c in zip(masks, counts)} == want
    names = [f"s{t}" for t in range(T)]
    assert qmc.relabel_tree(out, names) == "((((s1,s2)75,s3)0,s0)0,((s5,s4)25,(s6,s7)0));"
    with Consensus(T) as acc:
        acc.add_newick([qmc.relabel_tree(newick_of(A, T), names)] * 3, samples=names)
        assert acc.map_supports(qmc.relabel_tree(given, names), samples=names) == \
            "((((s1,s2)100,s3)0,s0)0,((s5,s4)0,(s6,s7)0));"


def test_relabel_tree_leaves_the_supports_alone():
    T = 12
    trees = cm.tree_set(T, seed=2)
    with Consensus(T) as acc:
        acc.add_parents(trees)
        nwk = acc.tree(0.2)
    names = {t: f"x{t}" for t in range(T)}
    named = qmc.relabel_tree(nwk, names)
    assert re.findall(r"\)(\d+)", named) == re.findall(r"\)(\d+)", nwk) and re.findall(r"\)(\d+)", nwk)
    assert re.sub(r"x(\d+)", r"\1", named) == nwk
    assert consensus_tree([newick_of(t, T) for t in trees], 0.2) == nwk
    assert consensus_tree([qmc.relabel_tree(newick_of(t, T), names) for t in trees], 0.2, samples=names) == named


def test_a_bad_tree_refuses_the_whole_add():
    T = 10
    good = cm.tree_set(T, seed=1)[:6]
    with Consensus(T) as acc:
        acc.add_parents(good)
        before = acc.raw()
        missing = np.array(good[0], np.int32)
        missing = np.append(missing, missing[3])                   # a second tip beside taxon 3 that is no taxon
        taken = np.array(good[1], np.int32)
        taken[4] = 5                                               # taxon 4 hangs below taxon 5
        for bad in (missing, taken):
            with pytest.raises(_lib.TetradHipError, match="tree 2"):
                acc.add_parents([good[0], good[1], bad, good[2]])
            for a, b in zip(before, acc.raw()):
                np.testing.assert_array_equal(a, b)
        with pytest.raises(ValueError, match="tree 1"):
            acc.add_newick(["((0,1),(2,3),(4,5),(6,7),(8,9));", "((0,1),(2,3),(4,5),(6,7),(8,8));"])
        with pytest.raises(ValueError, match="tree 0"):
            acc.add_newick(["((0,1),(2,3),(4,5),(6,7),8);"])
        for a, b in zip(before, acc.raw()):
            np.testing.assert_array_equal(a, b)


def test_max_splits_exceeded_is_an_error_and_reset_recovers():
    T = 16
    trees = cm.tree_set(T, seed=4)
    tab, n = cm.model_of(trees, T)
    with Consensus(T, max_splits=len(tab)) as acc:
        acc.add_parents(trees)
        cm.assert_matches(acc, tab, n, T)
    with Consensus(T, max_splits=len(tab) - 1) as acc:
        with pytest.raises(_lib.TetradHipError, match="max_splits"):
            acc.add_parents(trees)
            acc.raw()
        with pytest.raises(_lib.TetradHipError, match="max_splits"):
            acc.raw()
        acc.reset()
        acc.add_parents(trees[:4])
        cm.assert_matches(acc, *cm.model_of(trees[:4], T), T)


@pytest.mark.parametrize("T", [3, 4097])
def test_taxon_limits(lib, T):
    h = ctypes.c_void_p()
    assert lib.tq_cons_create(ctypes.byref(h), T, 100, None) == -1 and not h.value
    with pytest.raises(_lib.TetradHipError):
        Consensus(T)


@pytest.mark.parametrize("T", [63, 64, 65, 127, 128, 129])
def test_word_boundaries(T):
    """Sides that are every taxon but 0 and one tip: the complement of {0, x} under the tail mask of the last word."""
    trees = [quartet_tree(T, (0, x)) for x in (1, 62, 63, 64, T - 2, T - 1) if x < T]
    trees += cm.tree_set(T, seed=T)[:8]
    tab, n = check(trees, T, freqs=(0.5, 0.1))
    assert frozenset(range(1, T - 1)) in {s for s, _ in tab}
    with Consensus(T) as acc:
        acc.add_parents(trees)
        if T % 64:                                                 # the bits >= T of the last word stay clear
            assert not (acc.raw()[0][:, -1] >> np.uint64(T % 64)).any()


def test_run_consensus_end_to_end(tmp_path):
    from supertree_model import bipartitions, rows_from_tree
    from tetrad_amd.distributor import format_tsv
    T = 12
    files = []
    for i in range(6):
        children, root, q, sc, st = rows_from_tree(T, 400, "random", 0.05, seed=77, quartets=None)
        rng = np.random.default_rng(i)
        keep = rng.permutation(len(q))[:300]                       # every file sees another part of the rows
        f = tmp_path / f"rep{i}.tsv"
        f.write_text(format_tsv(q[keep], sc[keep], st[keep]))
        files.append(f)
    truth = {frozenset(range(T)) - s if 0 in s else s for s in bipartitions(children, root, T)}
    nwk = run_consensus(files, T)
    with Consensus(T) as acc:
        acc.add_newick([nwk])
        got = {frozenset(np.flatnonzero(m)) for m in acc.splits()[0]}
    assert got == truth
    assert all(0 <= int(x) <= 100 for x in re.findall(r"\)(\d+)", nwk))
    names = [f"sample_{t}" for t in range(T)]
    assert run_consensus(files, T, samples=names) == qmc.relabel_tree(nwk, names)
    mapped = run_consensus(files, T, tree=nwk)
    assert re.sub(r"\)\d+", ")", mapped) == re.sub(r"\)\d+", ")", nwk)
    assert sorted(re.findall(r"\)(\d+)", mapped)) == sorted(re.findall(r"\)(\d+)", nwk))
