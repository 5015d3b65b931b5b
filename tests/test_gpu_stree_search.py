"""GPU: the device execution of the exact integer cut search (`tq_stree_search_kernel`) equals the
plain-integer model bit for bit -- sides, cut flag and rounds -- and whole trees built under `search="exact"` on device
rows equal the host back end's string, whatever the graph pass form, wherever the search runs, and in the replicate
loops."""
import numpy as np
import pytest

import stree_search_model as model
from supertree_model import bad_rows, newick_bipartitions, rows_from_tree
from test_gpu_supertree import add_dev, to_dev
from tetrad_amd.qmc import Supertree, infer_supertree_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def big_node(n=1024, rows=60_000, seed=1024):
    """a node at the device limit: 10 % wrong rows of a random tree, weights 1-3"""
    _, _, q, sc, st = rows_from_tree(n, rows, "random", 0.1, seed=seed)
    q = np.asarray(q, np.int64)
    topo = np.asarray(st)[:, 0]
    sp = q.copy()
    sp[topo == 1] = q[topo == 1][:, [0, 2, 1, 3]]
    sp[topo == 2] = q[topo == 2][:, [0, 3, 1, 2]]
    k = 1 + np.arange(len(sp), dtype=np.uint64) % np.uint64(3)
    G = np.zeros(n * (n - 1) // 2, np.uint64)
    B = np.zeros_like(G)
    tri = lambda u, v: np.minimum(u, v) * n - np.minimum(u, v) * (np.minimum(u, v) + 1) // 2 + np.abs(u - v) - 1
    for M, pairs in ((B, ((0, 1), (2, 3))), (G, ((0, 2), (0, 3), (1, 2), (1, 3)))):
        for x, y in pairs:
            np.add.at(M, tri(sp[:, x], sp[:, y]), k)
    return ("big", n, G, B, model.node_seed(7, 0, 0))


def test_kernel_equals_the_model_on_a_mixed_batch(engine):
    """one launch, nodes of unequal size: 4, 5, 8, 9, 63, 64, 65, 128, 129 with every graph kind of the CPU test (the
    limit weights, zero B, zero G and ties among them), a refused random start, and one node of 1024"""
    cases = model.standard_cases([4, 5, 8, 9, 63, 64, 65, 128, 129])
    G, B = model.tree_graph(5, 40, 0.1, 55)
    cases.append(("forced", 5, G, B, model.forced_start_node(5)))
    cases.insert(len(cases) // 2, big_node())
    want = model.model_batch(cases)
    got = model.run_batch(cases, engine._h)
    assert got == model.run_batch(cases)                                    # the host execution
    for (name, n, *_), w, g in zip(cases, want, got):
        assert g == (w[0], w[1], w[2]), (name, n)
    big = [w for c, w in zip(cases, want) if c[0] == "big"][0]
    assert big[0] and big[2] >= 2                                           # the large node did run several rounds


def test_kernel_equals_the_model_on_300_small_nodes(engine):
    rng = np.random.default_rng(300)
    cases = []
    for i in range(300):
        n = 4 + i % 9                                                       # 4..12
        G, B = model.tree_graph(n, int(rng.integers(1, 8 * n)), float(rng.choice([0.0, 0.1, 0.4])), 1000 + i)
        if i % 50 == 49:
            B = np.zeros_like(B)
        cases.append((f"small{i}", n, G, B, model.node_seed(3, 1, i)))
    want = model.model_batch(cases)
    got = model.run_batch(cases, engine._h)
    for (name, n, *_), w, g in zip(cases, want, got):
        assert g == (w[0], w[1], w[2]), (name, n)
    assert sum(w[0] for w in want) > 200


TREES = [
    # T, rows, shape, wrong, strategy
    (4, 50, "random", 0.1, 1), (5, 200, "caterpillar", 0.0, 2), (9, 20_000, "random", 0.1, 0),
    (64, 20_000, "caterpillar", 0.1, 3), (65, 20_000, "random", 0.0, 1), (128, 20_000, "random", 0.1, 2),
    (128, 20_000, "caterpillar", 0.0, 0), (129, 20_000, "caterpillar", 0.1, 3), (300, 20_000, "random", 0.1, 1),
    (300, 20_000, "caterpillar", 0.0, 0), (1024, 200_000, "random", 0.1, 2),
]


@pytest.mark.parametrize("T,n,shape,wrong,weights", TREES)
def test_device_tree_equals_host_tree_under_exact(engine, T, n, shape, wrong, weights):
    """the same string and the same node counts per level, with the graph pass in both forms and the search on the
    device and on the host"""
    _, _, q, sc, st = rows_from_tree(T, n, shape, wrong, seed=T + weights)
    with Supertree(T, len(q), weights, engine=engine, search="exact") as dev, \
            Supertree(T, len(q), weights, search="exact") as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        want = host.tree(5)
        newick_bipartitions(want, T)
        try:
            for lds in (1, 0):
                for search_dev in (1, 0):
                    engine.set_option("stree_lds", lds)
                    engine.set_option("stree_search_dev", search_dev)
                    assert dev.tree(5) == want, (lds, search_dev)
                    assert dev.levels == host.levels
                    np.testing.assert_array_equal(dev.level_stats()[:, :3], host.level_stats()[:, :3])
        finally:
            engine.set_option("stree_lds", 1)
            engine.set_option("stree_search_dev", 1)


def test_bad_rows_reuse_two_streams_and_switching_rules(engine):
    import torch
    T, n = 40, 20_000
    rng = np.random.default_rng(5)
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.1, seed=3)
    bq, bsc, bst, bfl = bad_rows(T, 5000, rng)
    q, sc, st = np.concatenate([q, bq]), np.concatenate([sc, bsc]), np.concatenate([st, bst])
    fl = np.concatenate([np.zeros(n, np.uint8), bfl])
    perm = rng.permutation(len(q))
    q, sc, st, fl = q[perm], sc[perm], st[perm], fl[perm]
    d = to_dev(q, sc, st, fl)
    torch.cuda.synchronize()
    with Supertree(T, len(q), 1, min_snps=2, engine=engine) as dev, Supertree(T, len(q), 1, min_snps=2) as host:
        host.add(q, sc, st, fl)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        cuts = [0, 1, 64, 65, 4097, len(q)]
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):                  # adds on two streams
            add_dev(dev, d, lo, hi, stream=(s1, s2)[i & 1])
        assert host.counts()[1] >= 4000
        build = torch.cuda.Stream()
        f64 = host.tree(9)
        assert dev.tree(9, stream=build.cuda_stream) == f64                       # the accumulator as it was
        for acc in (dev, host):
            acc.set_search("exact")
        exact = host.tree(9)
        assert dev.tree(9, stream=build.cuda_stream) == exact
        assert dev.tree(2) == host.tree(2)
        for acc in (dev, host):
            acc.set_search("f64")
        assert dev.tree(9) == f64 == host.tree(9)                                 # f64 -> exact -> f64
        # reset and reuse with other rows under the exact rule
        _, _, q2, sc2, st2 = rows_from_tree(T, 8000, "balanced", 0.3, seed=13)
        for acc in (dev, host):
            acc.reset()
            acc.set_search("exact")
        add_dev(dev, to_dev(q2, sc2, st2))
        host.add(q2, sc2, st2)
        assert dev.tree(1) == host.tree(1) == infer_supertree_exact(q2, sc2, st2, T, weights=1, min_snps=2, seed=1,
                                                                      search="exact")
        torch.cuda.synchronize()


def test_replicate_loop_under_exact(engine):
    """bootstrap_trees(supertree="device", search="exact"): 3 replicates at 16 taxa equal the trees built by hand on the
    host back end from each replicate's rows"""
    from tetrad_amd import synth
    from tetrad_amd.replicates import ReplicateRunner, bootstrap_trees
    T, S, seed, Q, nboots = 16, 8000, 8, 1500, 3
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=seed, ambiguous=0.02)
    trees = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device",
                            search="exact")
    assert len(trees) == nboots
    rows = {}

    def on_result(k, S_, rstat, rscor, flags, quartets):
        rows[k] = (quartets.copy(), rscor.copy(), rstat.copy(), flags.copy())
    runner = ReplicateRunner(engine, seqarr, spans, Q, seed=21, quartets_to_host=True)
    runner.run(nboots, True, on_result=on_result)
    runner.close()
    for k in range(nboots):
        q, sc, st, fl = rows[k]
        assert trees[k] == infer_supertree_exact(q, sc, st, T, weights=1, seed=k, flags=fl, search="exact")
    with pytest.raises(ValueError, match="exact"):
        bootstrap_trees(engine, seqarr, spans, Q, 1, supertree="host", search="exact")


def test_species_loop_under_exact(engine):
    """bootstrap_species_trees(search="exact") at K = 8: the same strings from both of its back ends"""
    from species_alleles_model import LOOP_K, LOOP_SEED, loop_source
    from tetrad_amd import species
    seqarr, spans, sp, _ = loop_source()
    smap = species.SpeciesMap(sp, [f"clade{k}" for k in range(LOOP_K)])
    assert LOOP_K == 8
    dev = species.bootstrap_species_trees(engine, seqarr, spans, smap, 3, seed=LOOP_SEED, search="exact")
    host = species.bootstrap_species_trees(engine, seqarr, spans, smap, 3, seed=LOOP_SEED, supertree="host",
                                           search="exact")
    assert len(dev) == 3 and dev == host
    for nwk in dev:
        newick_bipartitions(nwk, LOOP_K)
