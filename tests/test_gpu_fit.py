"""GPU: the device execution of the quartet fit (`tq_fit_table_kernel` + `tq_fit_kernel` on device rows, DESIGN.md
section 17) equals the host execution and the split model of fit_model.py bit for bit -- over the table's LDS / L2
switch, the device limit, row counts around a wave and a workgroup, batches with duplicate trees, several chunks,
several adds, builds in between, a reset, the engine's own rows -- and best-of-N builds in the replicate loop."""
import functools

import numpy as np
import pytest

import fit_model as fm
from supertree_model import bad_rows, rows_from_tree, tree_children
from tetrad_amd.qmc import Supertree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def to_dev(q, sc, st, fl=None):
    import torch
    return (torch.tensor(q.view(np.int32)).cuda(), torch.tensor(st.view(np.int32)).cuda(),       # copies: the shared
            torch.tensor(sc).cuda(), None if fl is None else torch.tensor(fl).cuda())             # inputs are read-only


def add_dev(acc, d, lo=0, hi=None, stream=None):
    import torch
    dq, dst, dsc, dfl = d
    hi = dq.shape[0] if hi is None else hi
    s = torch.cuda.current_stream() if stream is None else stream
    acc.add_dev_ptrs(dq[lo:hi].data_ptr(), dst[lo:hi].data_ptr(), dsc[lo:hi].data_ptr(),
                     0 if dfl is None else dfl[lo:hi].data_ptr(), hi - lo, s.cuda_stream)


SHAPE = {4: "random", 5: "caterpillar", 128: "random", 129: "balanced", 300: "random", 1024: "balanced"}


@functools.lru_cache(maxsize=None)
def source(T):
    """100 000 rows of a generating tree, 10 % wrong, made once per T (the cases take the first n), and the candidate
    trees: polytomies, a star, the caterpillar (depth T - 1, the longest table walk), duplicates."""
    children, root, q, sc, st = rows_from_tree(T, 100_000, SHAPE[T], 0.1, seed=T)
    gen = fm.parent_from_children(children, root, T)
    rng = np.random.default_rng(T)
    cat = fm.parent_from_children(*tree_children(T, "caterpillar", None), T)
    other = fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(T + 1)), T)
    poly = fm.contract(gen, T, rng)
    trees = [poly, cat, poly, fm.star(T), gen, other, fm.contract(other, T, rng, 0.7), fm.root_on_edge(gen, 1)]
    for a in (q, sc, st, *trees):
        a.setflags(write=False)
    return q, sc, st, trees


def batch(T, R):
    trees = source(T)[3]
    return [trees[i % len(trees)] for i in range(R)]


def ints(res):
    """The six integers of every record, u64[R,6] (the fraction, NaN where nothing is resolved, left out)."""
    res = np.atleast_1d(res)
    return np.stack([res[f] for f in fm.FIELDS], axis=1)


def same(a, b):
    np.testing.assert_array_equal(ints(a), ints(b))
    np.testing.assert_array_equal(np.atleast_1d(a)["fraction"], np.atleast_1d(b)["fraction"])    # NaN equals NaN here


def check(dev, host, trees, model_trees=None):
    """device == host == model for `trees`; returns the device records"""
    rd, rh = dev.fit(trees), host.fit(trees)
    same(rd, rh)
    kept, _, sum_k = host.counts()
    assert dev.counts() == host.counts()
    sp, k = host.rows()
    for i in (range(len(trees)) if model_trees is None else model_trees):
        assert fm.as_ints(rd[i]) == fm.model_fit(trees[i], host.ntaxa, sp, k), i
    for r in rd:
        assert sum(fm.as_ints(r)[:3]) == sum_k and sum(fm.as_ints(r)[3:]) == kept
    return rd


CASES = [
    # T, kept rows, R, score scale (1280: k past 2^32 under strategy 1)
    (4, 1, 1, 1.0), (4, 63, 3, 1280.0), (4, 100_000, 17, 1.0), (5, 64, 1, 1.0), (5, 65, 17, 1.0), (5, 4097, 3, 1280.0),
    (128, 1, 3, 1.0), (128, 65, 1, 1.0), (128, 4097, 17, 1.0), (128, 100_000, 3, 1280.0),
    (129, 63, 1, 1.0), (129, 64, 3, 1280.0), (129, 4097, 17, 1.0), (129, 100_000, 3, 1.0),
    (300, 65, 3, 1.0), (300, 4097, 1, 1280.0), (300, 100_000, 17, 1.0),
    (1024, 1, 1, 1.0), (1024, 4097, 17, 1.0), (1024, 100_000, 3, 1280.0),
]


@pytest.mark.parametrize("T,n,R,scale", CASES)
def test_device_equals_host_and_model(engine, T, n, R, scale):
    q, sc, st, _ = source(T)
    q, sc, st = q[:n], sc[:n] * scale, st[:n]
    trees = batch(T, R)
    with Supertree(T, n, 1, engine=engine) as dev, Supertree(T, n, 1) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        assert host.counts()[0] == n
        # the model runs on the distinct trees of the batch (a duplicate is compared with its twin instead)
        rd = check(dev, host, trees, model_trees=range(min(R, 8 if n <= 4097 else 2)))
        if scale > 1:
            assert int(host.rows()[1].max()) >= 2**32
        if R >= 3:
            assert trees[0] is trees[2]
            same(rd[0], rd[2])                                              # duplicate trees, equal rows of out
        if R == 17:
            same(rd[:8], rd[8:16])
            if n >= 4097 and T >= 128:
                assert all(x > 0 for x in fm.as_ints(rd[0])), rd[0]         # a polytomous tree: all three classes


def test_no_kept_rows_on_the_device(engine):
    """device rows that the filters all drop: kept = 0, every tree scores zero"""
    T = 40
    bq, bsc, bst, bfl = bad_rows(T, 700, np.random.default_rng(1))
    with Supertree(T, 700, 1, engine=engine) as dev, Supertree(T, 700, 1) as host:
        add_dev(dev, to_dev(bq, bsc, bst, bfl))
        host.add(bq, bsc, bst, bfl)
        assert dev.counts() == host.counts() and dev.counts()[0] == 0
        trees = [fm.star(T), fm.parent_from_children(*tree_children(T, "balanced", None), T)]
        rd = check(dev, host, trees)
        assert all(fm.as_ints(r) == [0] * 6 for r in rd)
    with Supertree(T, 700, 1, engine=engine) as dev:                        # nothing added at all
        assert fm.as_ints(dev.fit(trees[1])) == [0] * 6


def test_three_chunks_equal_one(engine):
    """fit_scratch_bytes (read at an accumulator's first fit) that holds two tables: five trees take three chunks"""
    T, n = 129, 20_000
    q, sc, st, _ = source(T)
    q, sc, st = q[:n], sc[:n], st[:n]
    trees = batch(T, 8)[3:8]
    assert len(trees) == 5
    d = to_dev(q, sc, st)
    with Supertree(T, n, 1, engine=engine) as one, Supertree(T, n, 1, engine=engine) as three, Supertree(T, n, 1) as host:
        host.add(q, sc, st)
        add_dev(one, d)
        add_dev(three, d)
        want = check(one, host, trees)
        engine.set_option("fit_scratch_bytes", 2 * (2 * T * T) + 100)
        try:
            got = three.fit(trees)
        finally:
            engine.set_option("fit_scratch_bytes", 64 << 20)
        same(got, want)
        engine.set_option("fit_scratch_bytes", 1)                            # below one table: one tree per chunk
        try:
            with Supertree(T, n, 1, engine=engine) as single:
                add_dev(single, d)
                same(single.fit(trees), want)
        finally:
            engine.set_option("fit_scratch_bytes", 64 << 20)
        same(three.fit(trees[:1]), want[:1])                                # the bound is kept; smaller batches still run
        same(three.fit(trees + trees), np.concatenate([want, want]))        # the staging grows


def test_several_adds_builds_in_between_and_reuse(engine):
    import torch
    T, n = 128, 60_000
    q, sc, st, _ = source(T)
    q, sc, st = q[:n], sc[:n], st[:n]
    trees = batch(T, 5)
    d = to_dev(q, sc, st)
    torch.cuda.synchronize()
    with Supertree(T, n, 1, engine=engine) as one, Supertree(T, n, 1, engine=engine) as many, Supertree(T, n, 1) as host:
        host.add(q, sc, st)
        add_dev(one, d)
        s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        cuts = [0, 4097, 30_000, n]                                         # three adds on two streams
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            add_dev(many, d, lo, hi, stream=(s1, s2)[i & 1])
        want = check(one, host, trees)
        same(many.fit(trees, stream=s3.cuda_stream), want)
        # fit, build, fit: the root store is not modified, and the build is the one the host makes
        nwk = one.tree(9)
        assert nwk == host.tree(9)
        same(one.fit(trees), want)
        own = one.fit(nwk)
        same(own, host.fit(nwk))
        assert fm.as_ints(own)[2] == 0
        assert one.tree(9) == nwk
        # reset and reuse with other rows
        q2, sc2, st2 = rows_from_tree(T, 20_000, "balanced", 0.3, seed=13)[2:]
        one.reset()
        host.reset()
        assert fm.as_ints(one.fit(trees[0])) == [0] * 6
        add_dev(one, to_dev(q2, sc2, st2))
        host.add(q2, sc2, st2)
        check(one, host, trees)
        # a bad tree in the batch: refused with its index
        from tetrad_amd._lib import TetradHipError
        bad = np.append(trees[0], trees[0][3])
        with pytest.raises(TetradHipError, match="tree 1"):
            one.fit([trees[0], bad])
        check(one, host, trees[:2])
        torch.cuda.synchronize()


def test_best_of_n_on_device_rows(engine):
    T, n = 40, 20_000
    q, sc, st = rows_from_tree(T, n, "random", 0.4, seed=40)[2:]
    for search in ("f64", "exact"):
        with Supertree(T, n, 1, engine=engine, search=search) as dev, Supertree(T, n, 1, search=search) as host:
            add_dev(dev, to_dev(q, sc, st))
            host.add(q, sc, st)
            assert dev.tree(5, restarts=1) == dev.tree(5) == host.tree(5)
            best = dev.tree(5, restarts=4)
            assert best == host.tree(5, restarts=4)
            same(dev.last_fit.results, host.last_fit.results)
            assert dev.last_fit.chosen == host.last_fit.chosen
            singles = [host.tree(5 + i) for i in range(4)]
            assert best == singles[dev.last_fit.chosen]
            assert int(dev.last_fit.results[dev.last_fit.chosen]["k_satisfied"]) == max(
                int(r["k_satisfied"]) for r in host.fit(singles))
            np.testing.assert_array_equal(dev.level_stats()[:, :3], host.level_stats()[:, :3])


def test_from_the_engines_own_rows(engine):
    """c1 golden input resolved on the device -> add_dev_ptrs on the engine's output arrays -> fit, equal to the host
    execution and the model on the same rows copied out; the generating tree violates nothing it resolves wrongly"""
    import torch
    from tetrad_amd import synth
    tmparr, tmpmap, quartets = synth.make_config("c1")
    children, root = synth.random_tree_children(16, np.random.default_rng(synth.CONFIG_SEEDS["c1"]))
    gen = fm.parent_from_children(children, root, 16)
    Q = len(quartets)
    engine.set_data(tmparr, tmpmap)
    dq = torch.from_numpy(np.ascontiguousarray(quartets, np.uint32).view(np.int32)).cuda()
    drs = torch.empty((Q, 2), dtype=torch.int32, device="cuda")
    dsc = torch.empty((Q, 3), dtype=torch.float64, device="cuda")
    dfl = torch.empty(Q, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    engine.resolve_dev(dq.data_ptr(), Q, True, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), s)
    trees = [gen, fm.star(16), fm.contract(gen, 16, np.random.default_rng(0)), fm.reroot(gen, 20)]
    with Supertree(16, Q, 1, engine=engine) as dev, Supertree(16, Q, 1) as host:
        dev.add_dev_ptrs(dq.data_ptr(), drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), Q, s)
        nwk = dev.tree(0)
        rstat, rscor, flags = drs.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dfl.cpu().numpy()
        host.add(quartets, rscor, rstat, flags)
        rd = check(dev, host, trees)
        same(rd[0], rd[3])
        assert int(rd[0]["k_satisfied"]) > int(rd[0]["k_violated"])         # these rows rebuild the generating tree
        same(dev.fit(nwk), host.fit(nwk))


def test_replicate_loop_keeps_the_best_of_three(engine):
    """bootstrap_trees(supertree="device", restarts=3, fit_out=[]): each chosen tree is one of the three seed builds of
    that replicate's rows and satisfies the most weight of them; restarts=1 gives the strings it always gave"""
    from tetrad_amd import synth
    from tetrad_amd.replicates import ReplicateRunner, bootstrap_trees
    T, S, seed, Q, nboots = 24, 20_000, 8, 4000, 4
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=seed, ambiguous=0.02)
    f1, f3 = [], []
    plain = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device")
    trees1 = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device",
                             restarts=1, fit_out=f1)
    trees3 = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device",
                             restarts=3, fit_out=f3)
    assert plain == trees1 and len(trees3) == len(f3) == len(f1) == nboots
    rows = {}

    def on_result(k, S_, rstat, rscor, flags, quartets):
        rows[k] = (quartets.copy(), rscor.copy(), rstat.copy(), flags.copy())
    runner = ReplicateRunner(engine, seqarr, spans, Q, seed=21, quartets_to_host=True)
    runner.run(nboots, True, on_result=on_result)
    runner.close()
    for k in range(nboots):
        qk, sck, stk, flk = rows[k]
        with Supertree(T, len(qk), 1) as host:
            host.add(qk, sck, stk, flk)
            three = [host.tree(k + i) for i in range(3)]
            fits = host.fit(three)
            assert trees1[k] == three[0]                                    # what the loop gave before restarts existed
            same(f1[k], fits[0])
            assert trees3[k] in three
            assert int(f3[k]["k_satisfied"]) == max(int(r["k_satisfied"]) for r in fits)
            same(f3[k], host.fit(trees3[k]))
            assert trees3[k] == host.tree(k, restarts=3)
