"""GPU: the device execution of the exact supertree (`tq_stree_add_dev` + `tq_stree_build` on device rows) equals the
host execution bit for bit -- the kept rows (as sets: the device order is free), the root graph, and the newick STRING
-- over tree shapes, noise levels, weight strategies and sizes up to the device limit; from the engine's own rows; and
in the replicate loop (`bootstrap_trees(supertree="device")`)."""
import numpy as np
import pytest

from supertree_model import bad_rows, bipartitions, newick_bipartitions, rows_from_tree
from tetrad_amd.qmc import Supertree, infer_supertree_exact

pytestmark = pytest.mark.gpu
DEVICE_LIMIT = 1024


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def to_dev(q, sc, st, fl=None):
    import torch
    return (torch.from_numpy(q.view(np.int32)).cuda(), torch.from_numpy(st.view(np.int32)).cuda(),
            torch.from_numpy(sc).cuda(), None if fl is None else torch.from_numpy(fl).cuda())


def add_dev(acc, d, lo=0, hi=None, stream=None):
    import torch
    dq, dst, dsc, dfl = d
    hi = dq.shape[0] if hi is None else hi
    s = torch.cuda.current_stream() if stream is None else stream
    acc.add_dev_ptrs(dq[lo:hi].data_ptr(), dst[lo:hi].data_ptr(), dsc[lo:hi].data_ptr(),
                     0 if dfl is None else dfl[lo:hi].data_ptr(), hi - lo, s.cuda_stream)


def sorted_rows(acc):
    sp, k = acc.rows()
    rows = np.concatenate([sp.astype(np.uint64), k[:, None]], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def assert_same(dev, host, seed=5, min_levels=0):
    np.testing.assert_array_equal(sorted_rows(dev), sorted_rows(host))
    gd, gh = dev.graph(), host.graph()
    np.testing.assert_array_equal(gd[0], gh[0])
    np.testing.assert_array_equal(gd[1], gh[1])
    assert gd[2:] == gh[2:]
    td, th = dev.tree(seed), host.tree(seed)
    assert td == th
    assert dev.levels == host.levels >= min_levels
    np.testing.assert_array_equal(dev.level_stats()[:, :3], host.level_stats()[:, :3])   # nodes, live quartets, cells
    return td


CASES = [
    # T, rows, shape, wrong, strategy
    (4, 50, "random", 0.4, 1), (5, 200, "random", 0.1, 2), (16, 10_000, "balanced", 0.0, 0),
    (40, 10_000, "caterpillar", 0.4, 3), (128, 10_000, "random", 0.1, 1), (128, 10_000, "caterpillar", 0.4, 2),
    (128, 10_000, "balanced", 0.0, 0), (129, 10_000, "random", 0.1, 3), (300, 10_000, "caterpillar", 0.1, 1),
    (300, 10_000, "random", 0.4, 0), (DEVICE_LIMIT, 10_000, "random", 0.1, 2), (DEVICE_LIMIT, 10_000, "balanced", 0.0, 1),
]


@pytest.mark.parametrize("T,n,shape,wrong,weights", CASES)
def test_device_equals_host(engine, T, n, shape, wrong, weights):
    children, root, q, sc, st = rows_from_tree(T, n, shape, wrong, seed=T + weights)
    with Supertree(T, n, weights, engine=engine) as dev, Supertree(T, n, weights) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        nwk = assert_same(dev, host, min_levels=8 if T >= 128 else 0)
        newick_bipartitions(nwk, T)                                         # every taxon exactly once
        if wrong == 0.0 and T <= 40:
            assert newick_bipartitions(nwk, T) == bipartitions(children, root, T)


@pytest.mark.parametrize("shape,wrong,weights", [("random", 0.1, 1), ("caterpillar", 0.4, 0)])
def test_device_equals_host_at_a_million_rows(engine, shape, wrong, weights):
    T, n = 128, 1_000_000
    children, root, q, sc, st = rows_from_tree(T, n, shape, wrong, seed=77)
    with Supertree(T, n, weights, engine=engine) as dev, Supertree(T, n, weights) as host:
        d = to_dev(q, sc, st)
        add_dev(dev, d)
        host.add(q, sc, st)
        nwk = assert_same(dev, host, min_levels=8)
        if wrong <= 0.1:
            assert newick_bipartitions(nwk, T) == bipartitions(children, root, T)
        # the global-atomic form of the graph pass gives the same cells as the LDS form
        engine.set_option("stree_lds", 0)
        try:
            assert dev.tree(5) == nwk
            np.testing.assert_array_equal(dev.graph()[0], host.graph()[0])
        finally:
            engine.set_option("stree_lds", 1)


@pytest.mark.parametrize("weights", [0, 1, 2, 3])
def test_bad_rows_mixed_in(engine, weights):
    T, n = 40, 20_000
    rng = np.random.default_rng(weights)
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.2, seed=3)
    bq, bsc, bst, bfl = bad_rows(T, 5000, rng)
    q, sc, st = np.concatenate([q, bq]), np.concatenate([sc, bsc]), np.concatenate([st, bst])
    fl = np.concatenate([np.zeros(n, np.uint8), bfl])
    perm = rng.permutation(len(q))
    q, sc, st, fl = q[perm], sc[perm], st[perm], fl[perm]
    with Supertree(T, len(q), weights, min_snps=2, engine=engine) as dev, Supertree(T, len(q), weights, min_snps=2) as host:
        add_dev(dev, to_dev(q, sc, st, fl))
        host.add(q, sc, st, fl)
        assert_same(dev, host)
        assert host.counts()[1] >= 4000


def test_several_adds_on_two_streams_and_reuse(engine):
    import torch
    T, n = 128, 60_000
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.1, seed=12)
    d = to_dev(q, sc, st)
    torch.cuda.synchronize()
    with Supertree(T, n, 1, engine=engine) as one, Supertree(T, n, 1, engine=engine) as many, Supertree(T, n, 1) as host:
        host.add(q, sc, st)
        add_dev(one, d)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        cuts = [0, 1, 64, 65, 4097, 30_000, n]
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            add_dev(many, d, lo, hi, stream=(s1, s2)[i & 1])
        build = torch.cuda.Stream()
        ref = one.tree(9, stream=build.cuda_stream)
        assert many.tree(9, stream=build.cuda_stream) == ref == host.tree(9)
        assert_same(many, host, seed=2)
        assert one.tree(4) == host.tree(4) and one.tree(9) == ref             # a build leaves the rows intact
        # reset and reuse with other rows; capacity is enforced on the device path too
        _, _, q2, sc2, st2 = rows_from_tree(T, 20_000, "balanced", 0.3, seed=13)
        one.reset()
        host.reset()
        add_dev(one, to_dev(q2, sc2, st2))
        host.add(q2, sc2, st2)
        assert_same(one, host)
        from tetrad_amd._lib import TetradHipError
        with pytest.raises(TetradHipError, match="capacity"):
            add_dev(one, d)
        with pytest.raises(TetradHipError, match="do not mix"):
            one.add(q2, sc2, st2)
        assert_same(one, host)
        torch.cuda.synchronize()


def test_the_device_limit_is_refused_above(engine):
    from tetrad_amd._lib import TetradHipError
    with pytest.raises(TetradHipError, match="1024"):
        Supertree(DEVICE_LIMIT + 1, 10, engine=engine)
    with pytest.raises(TetradHipError):
        Supertree(3, 10, engine=engine)


@pytest.mark.parametrize("sub", [True, False])
def test_from_the_engines_own_rows(engine, sub):
    """c1 data resolved on the device -> add_dev_ptrs on the engine's output arrays -> the generating tree, equal to
    the host back end on the same rows copied out"""
    import torch
    from tetrad_amd import synth
    tmparr, tmpmap, quartets = synth.make_config("c1")
    children, root = synth.random_tree_children(16, np.random.default_rng(synth.CONFIG_SEEDS["c1"]))
    truth = bipartitions(children, root, 16)
    Q = len(quartets)
    engine.set_data(tmparr, tmpmap)
    dq = torch.from_numpy(np.ascontiguousarray(quartets, np.uint32).view(np.int32)).cuda()
    drs = torch.empty((Q, 2), dtype=torch.int32, device="cuda")
    dsc = torch.empty((Q, 3), dtype=torch.float64, device="cuda")
    dfl = torch.empty(Q, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    engine.resolve_dev(dq.data_ptr(), Q, sub, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), s)
    for weights in (0, 1, 2, 3):
        with Supertree(16, Q, weights, engine=engine) as dev:
            dev.add_dev_ptrs(dq.data_ptr(), drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), Q, s)
            nwk = dev.tree(0)
        assert newick_bipartitions(nwk, 16) == truth
        rstat, rscor, flags = drs.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dfl.cpu().numpy()
        assert nwk == infer_supertree_exact(quartets, rscor, rstat, 16, weights=weights, flags=flags)


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_replicate_loop_builds_the_trees_on_the_device(engine, sampler):
    """every tree of bootstrap_trees(supertree="device") equals the exact host path on that replicate's rows and
    carries every bipartition of the generating tree; concordance counts equal those of the supertree="host" run"""
    from concordance_model import random_tree
    from tetrad_amd import synth
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.replicates import ReplicateRunner, bootstrap_trees
    T, S, seed, Q, nboots = 24, 20_000, 8, 4000, 6
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=seed, ambiguous=0.02)
    children, root = synth.random_tree_children(T, np.random.default_rng(seed))
    truth = bipartitions(children, root, T)
    parent = random_tree(T, np.random.default_rng(4), multifurcate=0.2)
    conc = {}
    for mode in ("device", "host"):
        conc[mode] = Concordance(parent, ntaxa=T, min_snps=2, min_ratio=1.1, engine=engine)
        trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, sampler=sampler, workers=2,
                                concordance=conc[mode], supertree=mode)
        if mode == "device":
            dev_trees = trees
    assert len(dev_trees) == nboots
    rd, rh = conc["device"].raw(), conc["host"].raw()
    np.testing.assert_array_equal(rd["edge_counts"], rh["edge_counts"])
    np.testing.assert_array_equal(rd["tip_counts"], rh["tip_counts"])
    assert rd["skipped"] == rh["skipped"]
    rows = {}

    def on_result(k, S_, rstat, rscor, flags, quartets):
        rows[k] = (quartets.copy(), rscor.copy(), rstat.copy(), flags.copy())
    runner = ReplicateRunner(engine, seqarr, spans, Q, seed=21, sampler=sampler, quartets_to_host=True)
    runner.run(nboots, True, on_result=on_result)
    runner.close()
    for k in range(nboots):
        q, sc, st, fl = rows[k]
        assert dev_trees[k] == infer_supertree_exact(q, sc, st, T, weights=1, seed=k, flags=fl)
        assert truth <= newick_bipartitions(dev_trees[k], T), k
