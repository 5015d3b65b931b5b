"""GPU: the device execution of the NNI scan (`tq_nni_table_kernel` + `tq_nni_kernel` on device rows, DESIGN.md section
24) equals the host execution and the model of nni_model.py bit for bit -- over the table's LDS / L2 switch, the device
limit, row counts around a workgroup and a slice, one hot edge, polytomies, several adds, builds and fits in between, a
reset, the engine's own rows -- and polish gives one string and one trace from both back ends, in the replicate loop too."""
import functools

import numpy as np
import pytest

import fit_model as fm
import nni_model as nm
from supertree_model import bad_rows, rows_from_tree, sample_quartets, tree_children
from tetrad_amd.qmc import Supertree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


def to_dev(q, sc, st, fl=None):
    import torch
    return (torch.tensor(q.view(np.int32)).cuda(), torch.tensor(st.view(np.int32)).cuda(),
            torch.tensor(sc).cuda(), None if fl is None else torch.tensor(fl).cuda())


def add_dev(acc, d, lo=0, hi=None, stream=None):
    import torch
    dq, dst, dsc, dfl = d
    hi = dq.shape[0] if hi is None else hi
    s = torch.cuda.current_stream() if stream is None else stream
    acc.add_dev_ptrs(dq[lo:hi].data_ptr(), dst[lo:hi].data_ptr(), dsc[lo:hi].data_ptr(),
                     0 if dfl is None else dfl[lo:hi].data_ptr(), hi - lo, s.cuda_stream)


@functools.lru_cache(maxsize=None)
def source(T):
    """100 000 rows made once per T (the cases take the first n): half of the quartets drawn from all taxa, half from a
    window of 8 neighbouring taxa (neighbours in the balanced tree and the caterpillar, so that deep edges are met), every
    row with a random one of the three resolutions."""
    n = 100_000
    rng = np.random.default_rng(T)
    q = sample_quartets(T, n, rng)
    if T > 8:
        local = sample_quartets(8, n // 2, rng) + rng.integers(0, T - 7, n // 2).astype(np.uint32)[:, None]
        q[1::2] = local
    topo = rng.integers(0, 3, n)
    sc = rng.integers(2 * 64, 40 * 64, size=(n, 3)) / 64.0
    sc[np.arange(n), topo] = rng.integers(1, 2 * 64, n) / 64.0
    st = np.stack([topo, rng.integers(1, 3000, n)], axis=1).astype(np.uint32)
    for a in (q, sc, st):
        a.setflags(write=False)
    return q, sc, st


def edge_rows(par, T, n, seed):
    """n rows built from the tree: row i takes one random taxon from each corner of eligible edge i (cycling over the
    edges), in a random order and with a random one of the three resolutions, so every edge is met by every class and
    every corner taxon turns up as a and as b."""
    rng = np.random.default_rng(seed)
    eds = [e for e in nm.edges(nm.canonical(par, T), T) if e["eligible"]]
    taxa = [[[x for x in range(T) if m >> x & 1] for m in e["masks"]] for e in eds]
    q = np.empty((n, 4), np.uint32)
    for i in range(n):
        four = [c[int(rng.integers(len(c)))] for c in taxa[i % len(taxa)]]
        q[i] = rng.permutation(four)
    topo = rng.integers(0, 3, n)
    sc = rng.integers(2 * 64, 40 * 64, size=(n, 3)) / 64.0
    sc[np.arange(n), topo] = rng.integers(1, 2 * 64, n) / 64.0
    st = np.stack([topo, rng.integers(1, 3000, n)], axis=1).astype(np.uint32)
    return q, sc, st


@functools.lru_cache(maxsize=None)
def tree(T, shape):
    if shape == "polytomies":
        par = fm.contract(tree(T, "random"), T, np.random.default_rng(T))
    elif shape == "last_sibling":           # the caterpillar ((0,1),T-1),2),3)...: tip T - 1 is the sibling of node (0,1)
        children, nxt, cur = {}, T, 0
        for t in [1, T - 1] + list(range(2, T - 1)):
            children[nxt] = (cur, t)
            cur, nxt = nxt, nxt + 1
        par = fm.parent_from_children(children, cur, T)
    else:
        par = fm.parent_from_children(*tree_children(T, shape, np.random.default_rng(T + 7)), T)
    par.setflags(write=False)
    return par


def triple(rec):
    return [int(rec["w0"]), int(rec["w1"]), int(rec["w2"])]


def assert_scan_is_model(got, want):
    assert len(got) == len(want)
    for e, (g, (elig, masks, w)) in enumerate(zip(got, want)):
        assert bool(g["eligible"]) == elig and Supertree.corner_ints(g) == masks and triple(g) == w, e


CASES = [
    # T, tree, kept rows, model rows (0: device against host only)
    (5, "caterpillar", 257, 257), (8, "random", 4097, 4097), (8, "polytomies", 100_000, 100_000),
    (127, "random", 256, 256), (128, "balanced", 1, 1), (128, "random", 255, 255), (128, "random", 257, 257),
    (128, "polytomies", 4097, 4097), (128, "balanced", 100_000, 100_000),
    (129, "random", 1, 1), (129, "balanced", 256, 256), (129, "random", 257, 257), (129, "polytomies", 4097, 4097),
    (129, "balanced", 100_000, 100_000),
    (300, "random", 4097, 4097), (300, "polytomies", 100_000, 100_000),
    (1024, "balanced", 1, 1), (1024, "balanced", 100_000, 4097), (1024, "caterpillar", 100_000, 4097),
]


@pytest.mark.parametrize("T,shape,n,n_model", CASES)
def test_device_equals_host_and_model(engine, T, shape, n, n_model):
    par = tree(T, shape)
    if n <= 257:                            # few rows: built across the tree's edges, so that they count
        q, sc, st = edge_rows(par, T, n, seed=T + n)
    else:
        q, sc, st = source(T)
        q, sc, st = q[:n], sc[:n], st[:n]
    with Supertree(T, n, 1, engine=engine) as dev, Supertree(T, n, 1) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        assert host.counts()[0] == n and dev.counts() == host.counts()
        got, want = dev.nni_scan(par), host.nni_scan(par)
        np.testing.assert_array_equal(got, want)
        if n <= 257:
            met = [sum(triple(r)) > 0 for r in got]
            assert met[0] and (all(met) or n < len(got))
        if n_model == n:
            assert_scan_is_model(got, nm.model_scan(par, T, *host.rows()))
        else:
            with Supertree(T, n_model, 1, engine=engine) as part:
                add_dev(part, to_dev(q[:n_model], sc[:n_model], st[:n_model]))
                sp, k = host.rows()
                assert_scan_is_model(part.nni_scan(par), nm.model_scan(par, T, sp[:n_model], k[:n_model]))
        if n >= 4097:
            hit = sum(sum(triple(r)) for r in got)
            assert hit > 0
            if shape == "polytomies":
                assert 0 < int(got["eligible"].sum()) < len(got)
            else:
                assert len(got) == T - 3 and got["eligible"].all()


ODD = [(5, "last_sibling"), (7, "last_sibling"), (127, "last_sibling"), (5, "example"), (127, "random"), (129, "last_sibling")]


@pytest.mark.parametrize("T,shape", ODD)
def test_odd_taxon_counts_and_the_last_taxon_as_sibling(engine, T, shape):
    """Odd T has an odd number of u16 table entries, and the last one, L[T-1][T-1], is read when tip T - 1 is the sibling
    of an eligible edge below the root and a row pairs it across that edge: the table's LDS copy must hold it."""
    par = np.array([7, 7, 5, 5, 6, 6, 7, -1], np.int32) if shape == "example" else tree(T, shape)   # (0,1,((2,3),4))
    n = 24 * (T - 3)
    q, sc, st = edge_rows(par, T, n, seed=T)
    if shape != "random":
        last = (q[:, :2] == T - 1).any(axis=1)
        assert last.sum() >= 4 and len(set(st[last, 0].tolist())) == 3       # T - 1 as a or b, in every resolution
    with Supertree(T, n, 1, engine=engine) as dev, Supertree(T, n, 1) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        assert host.counts()[0] == n
        got = dev.nni_scan(par)
        np.testing.assert_array_equal(got, host.nni_scan(par))
        assert_scan_is_model(got, nm.model_scan(par, T, *host.rows()))
        assert len(got) == T - 3 and got["eligible"].all() and all(all(triple(r)) for r in got)
        np.testing.assert_array_equal(dev.nni_scan(par), got)               # again: nothing left over in LDS decides it
        assert dev.polish(par) == host.polish(par)


def test_one_edge_takes_every_row(engine):
    """T = 4: 100 000 copies of three rows with k near 2^41, all on the tree's only edge -- one hot LDS counter each"""
    T, n = 4, 100_000
    q = np.tile(np.array([[0, 1, 2, 3]], np.uint32), (n, 1))
    topo = (np.arange(n) % 3).astype(np.uint32)
    sc = 3.0e7 + np.tile((np.arange(n) % 5).astype(np.float64)[:, None], (1, 3))
    sc[np.arange(n), topo] = 1.0e7 + (np.arange(n) % 7)
    st = np.stack([topo, np.full(n, 100, np.uint32)], axis=1).astype(np.uint32)
    par = np.array([4, 4, 5, 5, -1, 4], np.int32)
    with Supertree(T, n, 1, engine=engine) as dev, Supertree(T, n, 1) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        sp, k = host.rows()
        assert len(k) == n and int(k.min()) >= 2**39 and sum(int(x) for x in k) < 2**64
        got = dev.nni_scan(par)
        np.testing.assert_array_equal(got, host.nni_scan(par))
        assert_scan_is_model(got, nm.model_scan(par, T, sp, k))
        assert len(got) == 1 and sum(triple(got[0])) == sum(int(x) for x in k) and all(triple(got[0]))


def test_no_kept_rows_on_the_device(engine):
    T = 40
    bq, bsc, bst, bfl = bad_rows(T, 700, np.random.default_rng(1))
    par = tree(T, "random")
    with Supertree(T, 700, 1, engine=engine) as dev, Supertree(T, 700, 1) as host:
        add_dev(dev, to_dev(bq, bsc, bst, bfl))
        host.add(bq, bsc, bst, bfl)
        assert dev.counts() == host.counts() and dev.counts()[0] == 0
        got = dev.nni_scan(par)
        np.testing.assert_array_equal(got, host.nni_scan(par))
        assert len(got) == T - 3 and got["eligible"].all() and not any(sum(triple(r)) for r in got)
        assert dev.polish(par) == host.polish(par) and dev.polish(par)[1].moves == []
    with Supertree(T, 700, 1, engine=engine) as dev:                        # nothing added at all
        assert not any(sum(triple(r)) for r in dev.nni_scan(par))


def test_several_adds_builds_in_between_and_reuse(engine):
    import torch
    T, n = 128, 60_000
    q, sc, st = source(T)
    q, sc, st = q[:n], sc[:n], st[:n]
    par = tree(T, "random")
    d = to_dev(q, sc, st)
    torch.cuda.synchronize()
    with Supertree(T, n, 1, engine=engine) as one, Supertree(T, n, 1, engine=engine) as many, Supertree(T, n, 1) as host:
        host.add(q, sc, st)
        add_dev(one, d)
        s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        cuts = [0, 4097, 30_000, n]                                         # three adds on two streams
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            add_dev(many, d, lo, hi, stream=(s1, s2)[i & 1])
        want = host.nni_scan(par)
        np.testing.assert_array_equal(many.nni_scan(par, stream=s3.cuda_stream), want)
        first = one.nni_scan(par)
        np.testing.assert_array_equal(first, want)
        # scan, build, fit, scan: the root store is not modified
        nwk = one.tree(9)
        assert nwk == host.tree(9)
        assert fm.as_ints(one.fit(nwk)) == fm.as_ints(host.fit(nwk))
        np.testing.assert_array_equal(one.nni_scan(par), first)
        np.testing.assert_array_equal(one.nni_scan(nwk), host.nni_scan(nwk))
        assert one.tree(9) == nwk
        # reset and reuse with other rows
        q2, sc2, st2 = source(127)
        q2, sc2, st2 = q2[:20_000], sc2[:20_000], st2[:20_000]
        one.reset()
        host.reset()
        assert not any(sum(triple(r)) for r in one.nni_scan(par))
        add_dev(one, to_dev(q2, sc2, st2))
        host.add(q2, sc2, st2)
        got = one.nni_scan(par)
        np.testing.assert_array_equal(got, host.nni_scan(par))
        assert any(sum(triple(r)) for r in got)
        from tetrad_amd._lib import TetradHipError
        with pytest.raises(TetradHipError, match="tree 0"):
            one.nni_scan(np.append(par, par[3]).astype(np.int32))
        np.testing.assert_array_equal(one.nni_scan(par), got)
        torch.cuda.synchronize()


@pytest.mark.parametrize("T,n", [(40, 20_000), (129, 30_000)])
def test_polish_on_the_device_is_polish_on_the_host(engine, T, n):
    q, sc, st = rows_from_tree(T, n, "random", 0.4, seed=T)[2:]
    start = tree(T, "random")
    with Supertree(T, n, 1, engine=engine) as dev, Supertree(T, n, 1) as host:
        add_dev(dev, to_dev(q, sc, st))
        host.add(q, sc, st)
        for first in (host.tree(5), start):
            got, want = dev.polish(first), host.polish(first)
            assert got == want
            nwk, trace = got
            assert trace.converged
            assert int(dev.fit(nwk)["k_satisfied"]) - int(dev.fit(first)["k_satisfied"]) == sum(trace.gains)
        assert sum(trace.gains) > 0 and len(trace.moves) >= 2                # the random start takes several rounds
        assert dev.polish(start, max_rounds=1) == host.polish(start, max_rounds=1)
        assert dev.tree(5, polish=True) == host.tree(5, polish=True) and dev.last_polish == host.last_polish
        assert dev.tree(5, restarts=3, polish=True) == host.tree(5, restarts=3, polish=True)
        assert dev.last_polish == host.last_polish and dev.last_fit.chosen == host.last_fit.chosen
        assert dev.tree(5) == host.tree(5) == dev.tree(5, polish=False)
        if T == 40:
            nwk, trace = dev.polish(start)
            assert (nwk, trace.moves, trace.gains, trace.converged) == nm.model_polish(start, T, *host.rows())


def test_from_the_engines_own_rows(engine):
    """c1 golden input resolved on the device -> add_dev_ptrs on the engine's output arrays -> scan and polish, equal to
    the host execution and the model on the same rows copied out"""
    import torch
    from tetrad_amd import synth
    tmparr, tmpmap, quartets = synth.make_config("c1")
    children, root = synth.random_tree_children(16, np.random.default_rng(synth.CONFIG_SEEDS["c1"]))
    gen = fm.parent_from_children(children, root, 16)
    other = tree(16, "random")
    Q = len(quartets)
    engine.set_data(tmparr, tmpmap)
    dq = torch.from_numpy(np.ascontiguousarray(quartets, np.uint32).view(np.int32)).cuda()
    drs = torch.empty((Q, 2), dtype=torch.int32, device="cuda")
    dsc = torch.empty((Q, 3), dtype=torch.float64, device="cuda")
    dfl = torch.empty(Q, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    engine.resolve_dev(dq.data_ptr(), Q, True, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), s)
    with Supertree(16, Q, 1, engine=engine) as dev, Supertree(16, Q, 1) as host:
        dev.add_dev_ptrs(dq.data_ptr(), drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), Q, s)
        rstat, rscor, flags = drs.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dfl.cpu().numpy()
        host.add(quartets, rscor, rstat, flags)
        assert dev.counts() == host.counts()
        sp, k = host.rows()
        for par in (gen, other):
            got = dev.nni_scan(par)
            np.testing.assert_array_equal(got, host.nni_scan(par))
            assert_scan_is_model(got, nm.model_scan(par, 16, sp, k))
            assert dev.polish(par) == host.polish(par)
        nwk, trace = dev.polish(other)
        assert (nwk, trace.moves, trace.gains, trace.converged) == nm.model_polish(other, 16, sp, k)
        assert sum(trace.gains) > 0


def test_replicate_loop_polishes_every_build(engine):
    """bootstrap_trees(supertree="device", polish=True, fit_out=[]) against builds, polishes and fits made by hand on
    each replicate's rows; polish=False gives the strings it always gave"""
    from tetrad_amd import synth
    from tetrad_amd.replicates import ReplicateRunner, bootstrap_trees
    T, S, seed, Q, nboots = 24, 20_000, 8, 4000, 3
    seqarr, maparr, spans = synth.make_c5_source(T=T, S=S, seed=seed, ambiguous=0.02)
    f0, fp = [], []
    plain = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device")
    off = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device",
                          polish=False, fit_out=f0)
    pol = bootstrap_trees(engine, seqarr, spans, Q, nboots, weights=1, seed=21, workers=2, supertree="device",
                          polish=True, fit_out=fp)
    assert plain == off and len(pol) == len(fp) == len(f0) == nboots
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
            build = host.tree(k)
            assert plain[k] == build
            assert fm.as_ints(f0[k]) == fm.as_ints(host.fit(build))
            nwk, trace = host.polish(build)
            assert pol[k] == nwk
            assert fm.as_ints(fp[k]) == fm.as_ints(host.fit(nwk))
            assert int(fp[k]["k_satisfied"]) - int(f0[k]["k_satisfied"]) == sum(trace.gains)
