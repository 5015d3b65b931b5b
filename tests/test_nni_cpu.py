"""CPU-only: the host execution of the NNI scan and the polish search (`tq_stree_nni_scan`, `tq_stree_polish` on host
rows) against the independent model of nni_model.py and against the quartet fit."""
import ctypes
import itertools

import numpy as np
import pytest

import fit_model as fm
import nni_model as nm
from supertree_model import bipartitions, newick_bipartitions, rows_from_tree, tree_children
from tetrad_amd import _lib
from tetrad_amd.qmc import PolishTrace, Supertree, infer_supertree_exact


@pytest.fixture(scope="module", autouse=True)
def built():
    _lib.build()


def triple(rec):
    return [int(rec["w0"]), int(rec["w1"]), int(rec["w2"])]


def assert_scan_is_model(got, want):
    assert len(got) == len(want)
    for e, (g, (elig, masks, w)) in enumerate(zip(got, want)):
        assert bool(g["eligible"]) == elig, e
        assert Supertree.corner_ints(g) == masks, e
        assert triple(g) == w, e


def rows(T, n, shape, wrong, seed, scale=1.0):
    """rows of a generating tree with all three resolutions, a fifth of them repeated; k is aligned with the rows"""
    children, root, q, sc, st = rows_from_tree(T, n, shape, wrong, seed)
    dup = np.arange(0, n, 5)
    q, sc, st = np.concatenate([q, q[dup]]), np.concatenate([sc, sc[dup]]) * scale, np.concatenate([st, st[dup]])
    return children, root, q, sc, st


def by_split(scan, T):
    """split of the edge (the side without taxon 0) -> (its two sides as sets of corner masks, w): what does not depend
    on the rooting"""
    out = {}
    for r in scan:
        if not r["eligible"]:
            continue
        x1, x2, y1, y2 = Supertree.corner_ints(r)
        side = x1 | x2 if not (x1 | x2) & 1 else y1 | y2
        assert side not in out
        out[side] = (frozenset([(x1, x2), (y1, y2)]), triple(r))
    return out


@pytest.mark.parametrize("shape", ["random", "balanced", "caterpillar"])
@pytest.mark.parametrize("T", [4, 5, 7, 16, 23, 40])
def test_scan_equals_the_model(T, shape):
    n = 600 if T >= 16 else 150
    children, root, q, sc, st = rows(T, n, shape, 0.4, seed=T + len(shape), scale=1280.0 if T in (7, 40) else 1.0)
    gen = fm.parent_from_children(children, root, T)
    other = fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(T)), T)
    with Supertree(T, len(q), 1) as acc:
        acc.add(q, sc, st)
        sp, k = acc.rows()
        assert len(set(st[:, 0].tolist())) == 3 or T == 4
        if T in (7, 40):
            assert int(k.max()) >= 2**32
        for tree in (gen, other):
            got = acc.nni_scan(tree)
            assert len(got) == T - 3 and got["eligible"].all()                # a binary tree
            assert_scan_is_model(got, nm.model_scan(tree, T, sp, k))
            assert sum(sum(triple(r)) for r in got) > 0


@pytest.mark.parametrize("T", [5, 9, 16])
def test_neighbour_identity_and_corners(T):
    """fit(neighbour) = fit(tree) shifted by the scanned weights, for every eligible edge and both alternatives"""
    children, root, q, sc, st = rows(T, 500, "random", 0.4, seed=100 + T)
    gen = fm.parent_from_children(children, root, T)
    with Supertree(T, len(q), 1) as acc:
        acc.add(q, sc, st)
        base = fm.as_ints(acc.fit(gen))
        scan = acc.nni_scan(gen)
        full = (1 << T) - 1
        for r in scan:
            m = Supertree.corner_ints(r)
            assert m[0] | m[1] | m[2] | m[3] == full and sum(bin(x).count("1") for x in m) == T    # a partition
            assert all(m)
        neigh = nm.all_neighbours(gen, T)
        assert len(neigh) == 2 * (T - 3)
        fits = acc.fit([p for _, _, p in neigh])
        for (e, alt, _), f in zip(neigh, fits):
            w = triple(scan[e])
            got = fm.as_ints(f)
            assert got[0] == base[0] - w[0] + w[alt], (e, alt)
            assert got[1] == base[1] + w[0] - w[alt], (e, alt)
            assert got[2] == base[2]


def test_other_writings_of_a_tree_scan_alike():
    T = 16
    children, root, q, sc, st = rows(T, 600, "random", 0.3, seed=77)
    gen = fm.parent_from_children(children, root, T)
    rng = np.random.default_rng(5)
    inner = [v for v in range(T, len(gen)) if gen[v] >= 0]
    with Supertree(T, len(q), 1) as acc:
        acc.add(q, sc, st)
        want = by_split(acc.nni_scan(gen), T)
        assert len(want) == T - 3
        writings = [fm.reroot(gen, v) for v in inner[:4]] + [fm.root_on_edge(gen, v) for v in (0, 5, inner[1], inner[-1])]
        writings.append(fm.subdivide(gen, [int(v) for v in rng.choice(len(gen) - 1, size=5, replace=False)
                                           if gen[int(v)] >= 0]))
        for tree in writings:
            assert by_split(acc.nni_scan(tree), T) == want


def test_polytomies_and_the_star():
    T = 23
    children, root, q, sc, st = rows(T, 600, "random", 0.4, seed=9)
    gen = fm.parent_from_children(children, root, T)
    poly = fm.contract(gen, T, np.random.default_rng(3))
    with Supertree(T, len(q), 1) as acc:
        acc.add(q, sc, st)
        sp, k = acc.rows()
        got = acc.nni_scan(poly)
        assert_scan_is_model(got, nm.model_scan(poly, T, sp, k))
        off = got[~got["eligible"]]
        assert 0 < len(off) < len(got) < T - 3
        assert not off["corners"].any() and not off["w0"].any() and not off["w1"].any() and not off["w2"].any()
        assert len(acc.nni_scan(fm.star(T))) == 0
        nwk, trace = acc.polish(fm.star(T))
        assert nwk == "(" + ",".join(str(i) for i in range(T)) + ");" and trace == PolishTrace([], [], True)
        # polishing a tree with polytomies moves only its eligible edges and resolves nothing
        nwk, trace = acc.polish(poly)
        want = nm.model_polish(poly, T, sp, k)
        assert (nwk, trace.moves, trace.gains, trace.converged) == want
        assert len(acc.nni_scan(nwk)) == len(got)


@pytest.mark.parametrize("search", ["f64", "exact"])
@pytest.mark.parametrize("T,wrong", [(12, 0.4), (23, 0.3), (40, 0.4)])
def test_polish_equals_the_model(T, wrong, search):
    children, root, q, sc, st = rows(T, 800, "random", wrong, seed=T)
    with Supertree(T, len(q), 1, search=search) as acc:
        acc.add(q, sc, st)
        sp, k = acc.rows()
        starts = [acc.tree(3), fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(T + 1)), T)]
        for start in starts:
            nwk, trace = acc.polish(start)
            want = nm.model_polish(acc._parent_of(start, None), T, sp, k)
            assert (nwk, trace.moves, trace.gains, trace.converged) == want
            assert trace.converged and len(trace.moves) == len(trace.gains)
            before, after = acc.fit(start), acc.fit(nwk)
            assert int(after["k_satisfied"]) - int(before["k_satisfied"]) == sum(trace.gains)
            assert int(before["k_violated"]) - int(after["k_violated"]) == sum(trace.gains)
            final = acc.nni_scan(nwk)
            assert all(max(w[1], w[2]) <= w[0] for w in map(triple, final))   # no candidate is left
            assert acc.polish(nwk) == (nwk, PolishTrace([], [], True))        # and the string is a fixed point
            if T == 12:
                par = acc._parent_of(nwk, None)
                top = fm.model_fit(par, T, sp, k)[0]
                neigh = nm.all_neighbours(par, T)
                assert len(neigh) == 2 * (T - 3)
                assert all(fm.model_fit(p, T, sp, k)[0] <= top for _, _, p in neigh)
        # the random start has something to gain; one round stops after one round
        assert sum(trace.gains) > 0 and len(trace.moves) >= 2
        one, t1 = acc.polish(starts[1], max_rounds=1)
        assert (t1.moves, t1.gains, t1.converged) == (trace.moves[:1], trace.gains[:1], False)
        assert int(acc.fit(one)["k_satisfied"]) - int(acc.fit(starts[1])["k_satisfied"]) == t1.gains[0]
        zero, t0 = acc.polish(starts[1], max_rounds=0)
        assert t0 == PolishTrace([], [], False)
        assert zero == nm.newick(nm.canonical(starts[1], T), T)
        assert fm.as_ints(acc.fit(zero)) == fm.as_ints(acc.fit(starts[1]))


@pytest.mark.parametrize("T,seed", [(T, s) for T in (8, 12, 16) for s in range(4)])
def test_one_round_restores_a_perturbed_tree(T, seed):
    """noise-free rows (every quartet, the generating tree's resolution, random k); the generating tree with one random
    interchange on each edge of a set of edges that share no node comes back in exactly one round"""
    quartets = np.array(list(itertools.combinations(range(T), 4)), np.uint32)
    children, root, q, sc, st = rows_from_tree(T, len(quartets), "random", 0.0, seed=1000 * T + seed, quartets=quartets)
    rng = np.random.default_rng(seed)
    gen = nm.canonical(fm.parent_from_children(children, root, T), T)
    eds = nm.edges(gen, T)
    used, start, moved = set(), gen, 0
    for e in rng.permutation(len(eds)):
        ed = eds[int(e)]
        if ed["u"] in used or ed["v"] in used:
            continue
        used.update((ed["u"], ed["v"]))
        start = nm.neighbour(start, T, ed, int(rng.integers(1, 3)))
        moved += 1
    assert moved >= 1
    with Supertree(T, len(q), 1) as acc:
        acc.add(q, sc, st)
        assert newick_bipartitions(acc.polish(start, max_rounds=0)[0], T) != bipartitions(children, root, T)
        nwk, trace = acc.polish(start)
        assert newick_bipartitions(nwk, T) == bipartitions(children, root, T)
        assert trace.moves == [moved] and trace.converged
        assert int(acc.fit(nwk)["k_violated"]) == 0


@pytest.fixture(scope="module")
def noisy40():
    T, n = 40, 4000
    return (T, n) + rows_from_tree(T, n, "random", 0.4, seed=40)[2:]


@pytest.mark.parametrize("search", ["f64", "exact"])
def test_polished_builds(noisy40, search):
    T, n, q, sc, st = noisy40
    with Supertree(T, n, 1, search=search) as acc:
        acc.add(q, sc, st)
        improved = 0
        for seed in range(8):
            plain = acc.tree(seed)
            assert acc.tree(seed, polish=False) == plain and acc.tree(seed, restarts=1, polish=False) == plain
            assert acc.last_polish is None
            pol = acc.tree(seed, polish=True)
            trace = acc.last_polish
            assert (pol, trace) == acc.polish(plain)
            a, b = int(acc.fit(plain)["k_satisfied"]), int(acc.fit(pol)["k_satisfied"])
            assert b >= a and b - a == sum(trace.gains)
            improved += b > a                                                # the next seed's plain build clears the trace
        assert improved >= 1
        # restarts with polish: the polished builds, chosen by the rule of `tree(restarts=N)`
        pols = [acc.polish(acc.tree(11 + i)) for i in range(4)]
        fits = acc.fit([p[0] for p in pols])
        best = acc.tree(11, restarts=4, polish=True)
        key = [(-int(r["k_satisfied"]), int(r["k_violated"]), i) for i, r in enumerate(fits)]
        chosen = key.index(min(key))
        assert acc.last_fit.chosen == chosen and best == pols[chosen][0] and acc.last_polish == pols[chosen][1]
        np.testing.assert_array_equal(acc.last_fit.results, fits)
        assert infer_supertree_exact(q, sc, st, T, weights=1, seed=11, search=search, restarts=4, polish=True) == best
        assert infer_supertree_exact(q, sc, st, T, weights=1, seed=2, search=search, polish=True) == \
            acc.tree(2, polish=True)
        assert infer_supertree_exact(q, sc, st, T, weights=1, seed=2, search=search, polish=False) == acc.tree(2)


def raw_scan(acc, parent, n_nodes, n_edges, elig, corners, w):
    return _lib.load().tq_stree_nni_scan(acc._h, parent.ctypes.data, n_nodes, None, ctypes.byref(n_edges),
                                         elig.ctypes.data, corners.ctypes.data, w.ctypes.data)


def raw_polish(acc, parent, n_nodes, max_rounds, buf, written, trace, rounds, conv):
    return _lib.load().tq_stree_polish(acc._h, parent.ctypes.data, n_nodes, max_rounds, None, buf.ctypes.data, len(buf),
                                       ctypes.byref(written), trace.ctypes.data, ctypes.byref(rounds), ctypes.byref(conv))


def test_a_bad_tree_is_refused_and_nothing_is_written():
    T = 10
    children, root, q, sc, st = rows_from_tree(T, 300, "random", 0.2, 8)
    good = fm.parent_from_children(children, root, T)
    missing = np.append(good, good[3]).astype(np.int32)                 # a second tip beside taxon 3 that is no taxon
    cycle = np.append(good, [len(good) + 1, len(good)]).astype(np.int32)     # two nodes that are each other's parent
    lib = _lib.load()
    with Supertree(T, 300, 1) as acc:
        acc.add(q, sc, st)
        # the single-tree calls take no stride: the node-count bound of the preparation stands in for it
        for bad, n_nodes, what in ((missing, len(missing), "no children"), (cycle, len(cycle), "cycle"),
                                   (good, 64 * 4096 + 1, "node count")):
            n_edges = ctypes.c_int64(-5)
            elig, corners, w = np.full(T, 9, np.uint8), np.full((T, 4, 1), 9, np.uint64), np.full((T, 3), 9, np.uint64)
            assert raw_scan(acc, bad, n_nodes, n_edges, elig, corners, w) == -1
            msg = lib.tq_last_error(None).decode()
            assert "tq_stree_nni_scan: tree 0" in msg and what in msg, msg
            assert n_edges.value == -5 and (elig == 9).all() and (corners == 9).all() and (w == 9).all()
            buf, trace = np.full(400, 9, np.uint8), np.full((5, 2), 9, np.uint64)
            written, rounds, conv = ctypes.c_int64(-5), ctypes.c_int64(-5), ctypes.c_int(-5)
            assert raw_polish(acc, bad, n_nodes, 5, buf, written, trace, rounds, conv) == -1
            msg = lib.tq_last_error(None).decode()
            assert "tq_stree_polish: tree 0" in msg and what in msg, msg
            assert (buf == 9).all() and (trace == 9).all() and (written.value, rounds.value, conv.value) == (-5, -5, -5)
        with pytest.raises(_lib.TetradHipError, match="tree 0"):
            acc.nni_scan(missing)
        with pytest.raises(_lib.TetradHipError, match="tree 0"):
            acc.polish(cycle)
        with pytest.raises(ValueError, match="taxa"):
            acc.nni_scan("((0,1),(2,3),4);")
        # max_rounds outside 0..65536
        buf, trace = np.full(400, 9, np.uint8), np.full((5, 2), 9, np.uint64)
        written, rounds, conv = ctypes.c_int64(-5), ctypes.c_int64(-5), ctypes.c_int(-5)
        for bad_rounds in (-1, 65537):
            assert raw_polish(acc, good, len(good), bad_rounds, buf, written, trace, rounds, conv) == -1
            assert "max_rounds" in lib.tq_last_error(None).decode()
            assert (buf == 9).all() and written.value == -5
            with pytest.raises(ValueError, match="max_rounds"):
                acc.polish(good, max_rounds=bad_rounds)
        # a buffer that is too small: the needed size, nothing else
        nwk, want = acc.polish(good)
        small = np.full(len(nwk) - 1, 9, np.uint8)
        assert raw_polish(acc, good, len(good), 5, small, written, trace, rounds, conv) == -6
        assert written.value == len(nwk) and (small == 9).all() and (trace == 9).all() and rounds.value == -5
        exact = np.full(len(nwk), 9, np.uint8)
        assert raw_polish(acc, good, len(good), 5, exact, written, trace, rounds, conv) == 0
        assert exact.tobytes().decode() == nwk and rounds.value == len(want.moves) and conv.value == 1
        # NULL outputs
        assert lib.tq_stree_nni_scan(acc._h, good.ctypes.data, len(good), None, None, None, None, None) == 0
        assert lib.tq_stree_polish(acc._h, good.ctypes.data, len(good), 5, None, exact.ctypes.data, len(exact),
                                   ctypes.byref(written), None, None, None) == 0
        assert_scan_is_model(acc.nni_scan(good), nm.model_scan(good, T, *acc.rows()))   # still usable


def test_a_sum_of_k_past_64_bits_is_refused():
    T, n = 8, 50_000
    children, root, q, sc, st = rows_from_tree(T, n, "random", 0.0, 4)
    gen = fm.parent_from_children(children, root, T)
    sc = np.full((n, 3), 3.9e9)
    with Supertree(T, n, 1) as acc:
        acc.add(q, sc, st)
        assert acc.counts()[2] == 2**64 - 1
        with pytest.raises(_lib.TetradHipError, match="64 bits"):
            acc.nni_scan(gen)
        with pytest.raises(_lib.TetradHipError, match="64 bits"):
            acc.polish(gen)
        assert acc.polish(gen, max_rounds=0)[0] == nm.newick(nm.canonical(gen, T), T)     # no scan, nothing to refuse


def test_no_rows_reset_and_reuse():
    T = 9
    children, root, q, sc, st = rows_from_tree(T, 200, "random", 0.3, 2)
    other = fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(1)), T)
    with Supertree(T, 200, 1) as acc:
        empty = acc.nni_scan(other)                                        # nothing added yet
        assert len(empty) == T - 3 and empty["eligible"].all() and not any(sum(triple(r)) for r in empty)
        assert acc.polish(other) == (nm.newick(nm.canonical(other, T), T), PolishTrace([], [], True))
        acc.add(q, sc, st)
        first = acc.nni_scan(other)
        assert_scan_is_model(first, nm.model_scan(other, T, *acc.rows()))
        acc.tree(3)                                                        # scans, builds and fits alternate
        acc.fit(other)
        np.testing.assert_array_equal(acc.nni_scan(other), first)
        acc.reset()
        np.testing.assert_array_equal(acc.nni_scan(other), empty)
        q2, sc2, st2 = rows_from_tree(T, 150, "balanced", 0.1, 3)[2:]
        acc.add(q2, sc2, st2)
        assert_scan_is_model(acc.nni_scan(other), nm.model_scan(other, T, *acc.rows()))


def test_polish_needs_the_device_supertree():
    from tetrad_amd.replicates import bootstrap_trees
    with pytest.raises(ValueError, match="polish"):
        bootstrap_trees(None, np.zeros((4, 8), np.uint8), np.zeros((1, 2), np.int64), 10, 1, supertree="host", polish=True)
