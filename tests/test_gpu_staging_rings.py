"""GPU: the two-piece page-locked staging rings behind the small host arrays of the device API -- the block boundaries
of ``patterns_blocks_dev``, the work items of ``taxon_counts_dev``, the locus draws (and packed starts) of ``bootstrap``.

A call copies its array into the next of two pieces and queues an H2D copy from it; the host waits only for the copy that
read that piece two calls ago.  So every case makes MORE back-to-back calls than there are pieces, with no synchronisation
between them, each with an array of its own (other values, other lengths) and outputs of its own, synchronises once, and
compares every output bitwise with a fresh engine that made that call alone: a piece overwritten while its copy was
queued, or a stale one, changes a result.  The last two cases release a ring while a copy out of it is queued
(``set_source`` of another source, closing the engine): both are legal, and the queued work must finish unharmed.

Shapes: T = 12 and S = 2 * TILE + 5 for the blocks and the taxon counts, 20 sets; the 10-taxon, 73-locus source of
test_gpu_bootstrap_layout.py and 64 quartets for the replicates."""
import numpy as np
import pytest

from test_gpu_bootstrap_layout import TILE, layout_source

pytestmark = pytest.mark.gpu

T, S = 12, 2 * TILE + 5
# five calls, B = 3, 1, 4, 2, 3: no two alike in value or (neighbours) in length
STARTS = [[3, TILE - 1, S - TILE + 7, S], [0, S], [1, 40, TILE, TILE + 33, S - 1], [TILE - 5, TILE + 5, S],
          [0, 31, 64, 2 * TILE]]
STREAMS = ["one stream", "two streams in turn"]


@pytest.fixture(scope="module")
def data():
    from tetrad_amd import synth
    return synth.simulate_tmparr(T, S, seed=71, missing=0.15)


@pytest.fixture(scope="module")
def sets():
    from tetrad_amd import synth
    return np.ascontiguousarray(synth.all_quartets(T)[:20], dtype=np.uint32)


@pytest.fixture(scope="module")
def sources():
    return layout_source(10, seed=12), layout_source(10, seed=14)


@pytest.fixture(scope="module")
def quartets10():
    from tetrad_amd import synth
    return np.ascontiguousarray(synth.all_quartets(10)[70:134], dtype=np.uint32)


def streams_for(how, n):
    import torch
    pool = [torch.cuda.Stream() for _ in range(1 if how == STREAMS[0] else 2)]
    return [pool[i % len(pool)].cuda_stream for i in range(n)], pool


def device_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def filled(*shape):
    import torch
    return torch.full(shape, -1, dtype=torch.int32, device="cuda")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("how", STREAMS)
def test_block_boundaries_of_five_queued_calls(data, sets, how):
    import torch
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as F:
        F.set_data(*data)
        want = [F.patterns_blocks(sets, b) for b in STARTS]
    with QuartetEngine(0) as E:
        E.set_data(*data)
        d_sets = device_u32(sets)
        outs = [filled(len(sets), len(b) - 1, 16) for b in STARTS]
        st, keep = streams_for(how, len(STARTS))
        torch.cuda.synchronize()
        for b, out, s in zip(STARTS, outs, st):
            E.patterns_blocks_dev(d_sets.data_ptr(), len(sets), b, out.data_ptr(), s)
        torch.cuda.synchronize()
        for i, (out, w) in enumerate(zip(outs, want)):
            np.testing.assert_array_equal(host_u32(out), w, err_msg=f"call {i}, B={len(STARTS[i]) - 1}, {how}")
            assert w[:, :, 15].sum() > 0


@pytest.mark.parametrize("how", STREAMS)
def test_work_items_of_five_queued_taxon_counts(data, how):
    import torch
    from tetrad_amd import distance
    from tetrad_amd.engine import QuartetEngine
    want = [distance.taxon_counts_host(data[0], b) for b in STARTS]
    with QuartetEngine(0) as E:
        E.set_data(*data)
        outs = [filled(len(b) - 1, T, T, 4) for b in STARTS]
        st, keep = streams_for(how, len(STARTS))
        torch.cuda.synchronize()
        for b, out, s in zip(STARTS, outs, st):
            E.taxon_counts_dev(b, out.data_ptr(), s)
        torch.cuda.synchronize()
        for i, (out, w) in enumerate(zip(outs, want)):
            np.testing.assert_array_equal(host_u32(out), w, err_msg=f"call {i}, B={len(STARTS[i]) - 1}, {how}")
            assert w[..., 1].sum() > 0


def five_draws(spans, seed):
    """Five draws of the loci with replacement, the longest replicate first (the layout buffers are allocated once, so no
    later call waits for the device), each with its seeds."""
    rng = np.random.default_rng(seed)
    n = len(spans)
    draws = [rng.integers(0, n, size=n).astype(np.int64) for _ in range(5)]
    draws.sort(key=lambda d: -int((spans[d, 1] - spans[d, 0]).sum()))
    assert len({int((spans[d, 1] - spans[d, 0]).sum()) for d in draws}) == 5
    return [(d, 100 + i, 200 + i) for i, d in enumerate(draws)]


def replicate_rows(eng, reps, quartets, stream):
    """bootstrap + resolve_dev (subsample mode: it reads the packed set under boot_pack) for every replicate of `reps`, back
    to back on `stream`, each into outputs of its own; one synchronisation at the end."""
    import torch
    d_q = device_u32(quartets)
    Q = len(quartets)
    outs = [(filled(Q, 2), torch.full((Q, 3), -1.0, dtype=torch.float64, device="cuda"),
             torch.full((Q,), 255, dtype=torch.uint8, device="cuda")) for _ in reps]
    torch.cuda.synchronize()
    for (lidxs, s1, s2), (rstat, rscor, flags) in zip(reps, outs):
        eng.bootstrap(lidxs, s1, s2, stream=stream.cuda_stream)
        eng.resolve_dev(d_q.data_ptr(), Q, True, rstat.data_ptr(), rscor.data_ptr(), flags.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    return [(host_u32(rstat), rscor.cpu().numpy(), flags.cpu().numpy()) for rstat, rscor, flags in outs]


def assert_rows_bitwise(got, want, what):
    for name, a, b in zip(("rstat", "rscor", "flags"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name}"
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{what}: {name}")


def fresh_replicate_rows(src, rep, quartets, boot_pack):
    import torch
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as F:
        F.set_option("boot_pack", boot_pack)
        F.set_source(*src)
        return replicate_rows(F, [rep], quartets, torch.cuda.Stream())[0]


@pytest.mark.parametrize("boot_pack", [0, 1])
def test_draws_of_five_queued_replicates(sources, quartets10, boot_pack):
    import torch
    from tetrad_amd.engine import QuartetEngine
    src = sources[0]
    reps = five_draws(src[1], seed=5)
    with QuartetEngine(0) as E:
        E.set_option("boot_pack", boot_pack)
        E.set_source(*src)
        got = replicate_rows(E, reps, quartets10, torch.cuda.Stream())
        assert E.site_pack_state()[1] == bool(boot_pack)
    rows = [fresh_replicate_rows(src, rep, quartets10, boot_pack) for rep in reps]
    for i, (g, w) in enumerate(zip(got, rows)):
        assert_rows_bitwise(g, w, f"replicate {i}, boot_pack={boot_pack}")
    assert any(not np.array_equal(rows[0][0], r[0]) for r in rows[1:])         # the replicates do differ


def test_set_source_while_a_draw_is_queued(sources, quartets10):
    import torch
    from tetrad_amd.engine import QuartetEngine
    first, second = sources
    rep = five_draws(second[1], seed=6)[0]
    with QuartetEngine(0) as E:
        E.set_source(*first)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        E.bootstrap(*five_draws(first[1], seed=7)[0], stream=s.cuda_stream)
        E.set_source(*second)                                   # releases the staging pieces of the first source
        got = replicate_rows(E, [rep], quartets10, s)[0]
    assert_rows_bitwise(got, fresh_replicate_rows(second, rep, quartets10, 0), "second source")


def test_close_while_block_boundaries_are_queued(data, sets):
    import torch
    from tetrad_amd.engine import QuartetEngine
    b = STARTS[2]
    with QuartetEngine(0) as F:
        F.set_data(*data)
        want = F.patterns_blocks(sets, b)
    E = QuartetEngine(0)
    E.set_data(*data)
    d_sets, out = device_u32(sets), filled(len(sets), len(b) - 1, 16)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    E.patterns_blocks_dev(d_sets.data_ptr(), len(sets), b, out.data_ptr(), s.cuda_stream)
    E.close()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_u32(out), want)
    with QuartetEngine(0) as N:                                 # the released pieces are in the pool: a new engine takes them
        N.set_data(*data)
        np.testing.assert_array_equal(N.patterns_blocks(sets, b), want)
