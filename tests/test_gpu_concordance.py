"""GPU: the concordance kernel (`tq_conc_add_dev`) equals the host accumulator on the same rows -- integer counters
bit-exact, the weight / score sums within 1e-12 relative -- on the LDS-table path (T = 128) and the global-table path
(T = 600); the replicate loop feeds it every replicate's rows; two ranks reduce to one.

At the sizes where `tree_acc_add_dev` changes form (T = 129, 255, 256: the 256-taxon LDS form; 257: the global-table form),
where that form starts a second edge pass (2 051 taxa = 2 048 edges = one full pass, 2 052 = a second pass of one
edge) and at the table limit (4 096: two passes, fewer slabs than CUs) the device is compared with the split-mask
model of tests/concordance_split_model.py, which shares nothing with the library's tree tables, on rows aimed at
every edge."""
import functools
import ctypes
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from concordance_model import random_tree
from concordance_split_model import (SplitModel, assert_raw_matches, caterpillar, dress_rows, mixed_rows,
                                     targeted_rows)

REPO = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu


def rows(T, n, rng):
    """Random rows (unsorted positions) with every flag, repeated / out-of-range taxa, rounding ties and scores on
    the min_ratio = 1.25 boundary."""
    q = rng.integers(0, T, size=(n, 4)).astype(np.uint32)          # unsorted; a few repeat a taxon (skipped)
    sc = rng.uniform(0.0, 400.0, size=(n, 3))
    k = rng.random(n)
    sc[k < 0.1] = rng.integers(0, 400 * 128, size=(int((k < 0.1).sum()), 3)) / 128.0      # 6-decimal ties
    b = (k >= 0.1) & (k < 0.2)
    sc[b] = np.array([1.0, 1.25, 1.25]) * rng.integers(1, 100, size=(int(b.sum()), 1))      # score == 1.25 exactly
    sc[(k >= 0.2) & (k < 0.22)] = 0.0
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 40, n)], axis=1).astype(np.uint32)
    fl = np.zeros(n, np.uint8)
    m = rng.random(n)
    fl[m < 0.05] = rng.choice([1, 2, 4, 8, 16], size=int((m < 0.05).sum()))
    q[(m >= 0.05) & (m < 0.06), 3] = q[(m >= 0.05) & (m < 0.06), 0]
    q[(m >= 0.06) & (m < 0.07), 1] = T + 3
    return q, sc, st, fl


def to_dev(q, sc, st, fl):
    import torch
    return (torch.from_numpy(q.view(np.int32)).cuda(), torch.from_numpy(st.view(np.int32)).cuda(),
            torch.from_numpy(sc).cuda(), torch.from_numpy(fl).cuda())


def assert_same(a, b):
    ra, rb = a.raw(), b.raw()
    np.testing.assert_array_equal(ra["edge_counts"], rb["edge_counts"])
    np.testing.assert_array_equal(ra["tip_counts"], rb["tip_counts"])
    assert ra["skipped"] == rb["skipped"]
    np.testing.assert_allclose(ra["edge_sums"], rb["edge_sums"], rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


@pytest.mark.parametrize("T", [128, 600])
def test_device_equals_host(engine, T):
    import torch
    from tetrad_amd.concordance import Concordance
    rng = np.random.default_rng(T)
    parent = random_tree(T, rng, multifurcate=0.15)
    for n in (1, 63, 64, 65, 4097, 1_000_000):
        q, sc, st, fl = rows(T, n, rng)
        dev = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25, engine=engine)
        host = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25)
        dq, dst, dsc, dfl = to_dev(q, sc, st, fl)
        dev.add_dev(dq, dst, dsc, dfl)
        host.add(q, sc, st, fl)
        assert_same(dev, host)
        # the same rows without the flags array, on a side stream
        dev.reset()
        host.reset()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        dev.add_dev(dq, dst, dsc, None, stream=s)
        host.add(q, sc, st)
        assert_same(dev, host)
        torch.cuda.synchronize()
        if n == 1_000_000:
            assert host.raw()["edge_counts"][:, 1:5].sum() > n // 10
        dev.close()


def test_two_adds_equal_one_add(engine):
    from tetrad_amd.concordance import Concordance
    rng = np.random.default_rng(2)
    T = 128
    parent = random_tree(T, rng)
    q, sc, st, fl = rows(T, 30001, rng)
    one = Concordance(parent, ntaxa=T, engine=engine)
    two = Concordance(parent, ntaxa=T, engine=engine)
    d = to_dev(q, sc, st, fl)
    one.add_dev(*d)
    h = 12345
    two.add_dev(d[0][:h], d[1][:h], d[2][:h], d[3][:h])
    two.add_dev(d[0][h:], d[1][h:], d[2][h:], d[3][h:])
    r1, r2 = one.raw(), two.raw()
    np.testing.assert_array_equal(r1["edge_counts"], r2["edge_counts"])
    np.testing.assert_array_equal(r1["tip_counts"], r2["tip_counts"])
    np.testing.assert_allclose(r1["edge_sums"], r2["edge_sums"], rtol=1e-12)
    # repeatable run to run: integer counters bit-exact
    one.reset()
    one.add_dev(*d)
    np.testing.assert_array_equal(one.raw()["edge_counts"], r1["edge_counts"])


@pytest.mark.parametrize("sampler", ["host", "device"])
def test_replicate_loop_feeds_the_accumulator(engine, sampler):
    from tetrad_amd import synth
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.replicates import ReplicateRunner
    seqarr, maparr, spans = synth.make_c5_source(T=14, S=6000, seed=8, ambiguous=0.02)
    rng = np.random.default_rng(4)
    parent = random_tree(14, rng, multifurcate=0.2)
    dev = Concordance(parent, ntaxa=14, min_snps=2, min_ratio=1.1, engine=engine)
    host = Concordance(parent, ntaxa=14, min_snps=2, min_ratio=1.1)
    runner = ReplicateRunner(engine, seqarr, spans, 701, seed=5, sampler=sampler, pieces=2, quartets_to_host=True,
                             concordance=dev)
    seen = []

    def on_result(k, S, rstat, rscor, flags, quartets):
        seen.append(k)
        host.add(quartets, rscor, rstat, flags)
    runner.run(3, True, on_result=on_result)
    runner.close()
    assert seen == [0, 1, 2]
    assert_same(dev, host)
    assert dev.raw()["edge_counts"][:, 1:5].sum() > 0


WORKER = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch, torch.distributed as dist
rank, world, port, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
from concordance_model import random_tree
from concordance_split_model import (SplitModel, assert_raw_matches, caterpillar, dress_rows, mixed_rows,
                                     targeted_rows)
from tetrad_amd import synth
from tetrad_amd.concordance import Concordance
from tetrad_amd.resolve_quartets import get_engine
from tetrad_amd.replicates import ReplicateRunner
seqarr, maparr, spans = synth.make_c5_source(T=14, S=6000, seed=8, ambiguous=0.02)
parent = random_tree(14, np.random.default_rng(4), multifurcate=0.2)
acc = Concordance(parent, ntaxa=14, min_snps=2, min_ratio=1.1, engine=get_engine(0))
runner = ReplicateRunner(get_engine(0), seqarr, spans, 701, seed=5, sampler="host", pieces=2, concordance=acc)
runner.run(3, True)
runner.close()
r = acc.raw()
np.savez(out + f".{rank}.npz", counts=r["edge_counts"], sums=r["edge_sums"], tips=r["tip_counts"], skipped=r["skipped"])
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_equal_one_rank(engine, tmp_path):
    from tetrad_amd import synth
    from tetrad_amd.concordance import Concordance
    from tetrad_amd.replicates import ReplicateRunner
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    out = str(tmp_path / "conc")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(REPO), str(r), "2", port, out], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    seqarr, maparr, spans = synth.make_c5_source(T=14, S=6000, seed=8, ambiguous=0.02)
    parent = random_tree(14, np.random.default_rng(4), multifurcate=0.2)
    one = Concordance(parent, ntaxa=14, min_snps=2, min_ratio=1.1, engine=engine)
    runner = ReplicateRunner(engine, seqarr, spans, 701, seed=5, sampler="host", concordance=one)
    runner.run(3, True)
    runner.close()
    r = one.raw()
    z0, z1 = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    np.testing.assert_array_equal(z0["counts"], r["edge_counts"])
    np.testing.assert_array_equal(z0["tips"], r["tip_counts"])
    assert int(z0["skipped"]) == r["skipped"]
    np.testing.assert_allclose(z0["sums"], r["edge_sums"], rtol=1e-12)
    assert (z1["counts"][:, 1:] == 0).all()                    # the other rank handed its counts over
    assert r["edge_counts"][:, 1:5].sum() > 0


def test_bad_arguments_are_error_codes(engine):
    import torch
    from tetrad_amd import _lib
    from tetrad_amd.concordance import Concordance
    lib = _lib.load()
    acc = Concordance("((0,1),(2,3),(4,5));", engine=engine)
    d = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
    assert lib.tq_conc_add_dev(acc._h, d.data_ptr(), None, d.data_ptr(), None, 4, None) == -1
    assert lib.tq_conc_add_dev(acc._h, d.data_ptr(), d.data_ptr(), d.data_ptr(), None, -1, None) == -1
    assert lib.tq_conc_add_dev(None, d.data_ptr(), d.data_ptr(), d.data_ptr(), None, 4, None) == -1
    assert b"tq_conc_add_dev" in lib.tq_last_error(engine._h)
    assert lib.tq_conc_add_dev(acc._h, None, None, None, None, 0, None) == 0            # nothing to add
    h = ctypes.c_void_p()
    par = np.array([4, 4, 4, 4, 4], np.int32)                                           # no root
    assert lib.tq_conc_create(ctypes.byref(h), par.ctypes.data, 5, 4, 0, 1.0, engine._h) == -1
    assert b"tq_conc_create" in lib.tq_last_error(engine._h)
    with pytest.raises(ValueError):
        acc.add_dev(d, d[:, :2].contiguous(), torch.zeros((3, 3), dtype=torch.float64, device="cuda"))
    r = acc.raw()
    assert r["edge_counts"][:, 1:].sum() == 0 and r["skipped"] == 0


# -- the kernel forms and edge passes against the split model ---------------------------------------------------------
K_TARGET = 4
N_RANDOM = 50_000
BIG_CASES = [(129, "binary"), (255, "binary"), (256, "binary"), (257, "binary"), (2051, "binary"), (2052, "binary"),
             (4096, "binary"), (4096, "multifurcating"), (4096, "caterpillar")]


def big_tree(T, shape):
    rng = np.random.default_rng([T, len(shape)])
    if shape == "caterpillar":
        return caterpillar(T)
    return random_tree(T, rng, multifurcate=0.15 if shape == "multifurcating" else 0.0,
                       rooted=shape != "multifurcating")


@functools.lru_cache(maxsize=None)
def big_case(T, shape):
    """(parent, model with both row sets added, targeted rows, random rows, random rows induced on an edge)."""
    rng = np.random.default_rng([T, len(shape), 1])
    parent = big_tree(T, shape)
    model = SplitModel(parent, T, 3, 1.25)
    tq, target = targeted_rows(model.masks, T, K_TARGET, rng, family=model.family)
    aimed = dress_rows(tq, rng)
    rand = mixed_rows(T, N_RANDOM, rng, window=8 if shape == "caterpillar" else None)
    model.add(*aimed)
    assert model.rows_induced == len(tq) == K_TARGET * model.E
    model.add(*rand)
    return parent, model, aimed, rand, model.rows_induced - len(tq)


@pytest.mark.parametrize("T, shape", BIG_CASES)
def test_device_equals_split_model(engine, T, shape):
    import torch
    from tetrad_amd.concordance import Concordance
    parent, model, aimed, rand, rand_induced = big_case(T, shape)
    dev = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25, engine=engine)
    host = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25)
    if shape != "multifurcating":
        assert dev.n_edges == T - 3                   # 2 051 taxa: exactly one full pass of 2 048 edges
    for r in (aimed, rand):
        dev.add_dev(*to_dev(*r))
        host.add(*r)
    idx, raw, res = assert_raw_matches(dev, model)    # every row of both sets: no row is left out
    assert_raw_matches(host, model)
    assert_same(dev, host)
    # what keeps the comparison honest
    counted = raw["edge_counts"][:, 1:5].sum(1)
    assert (res["counted"] >= K_TARGET).all()
    assert (counted >= K_TARGET).all()
    if T >= 2052:
        assert dev.n_edges > 2048 and (counted[2048:] >= K_TARGET).all()       # the edges of the second pass
    assert rand_induced >= 0.15 * N_RANDOM, rand_induced
    # the 1 000 000-row case against the host accumulator: with the flags array, then without it on a side stream
    rng = np.random.default_rng([T, len(shape), 2])
    q, sc, st, fl = mixed_rows(T, 1_000_000, rng, window=8 if shape == "caterpillar" else None)
    dq, dst, dsc, dfl = to_dev(q, sc, st, fl)
    dev.add_dev(dq, dst, dsc, dfl)
    host.add(q, sc, st, fl)
    assert_same(dev, host)
    dev.reset()
    host.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    for r in (aimed, rand):
        d = to_dev(*r)
        dev.add_dev(d[0], d[1], d[2], None, stream=s)
        host.add(*r[:3])
    dev.add_dev(dq, dst, dsc, None, stream=s)
    host.add(q, sc, st)
    assert_same(dev, host)
    torch.cuda.synchronize()
    assert host.raw()["edge_counts"][:, 1:5].sum() > 1_000_000 // 10
    dev.close()


@pytest.mark.parametrize("T, shape", [(256, "binary"), (4096, "binary")])
def test_two_adds_equal_one_add_at_size(engine, T, shape):
    """900 000 rows (as many workgroups as the slab or the device allows), then 3 000 rows (one workgroup): the fold
    of the second add must take that add's slabs only."""
    from tetrad_amd.concordance import Concordance
    parent, model, aimed, rand, _ = big_case(T, shape)
    rng = np.random.default_rng([T, 3])
    big = mixed_rows(T, 900_000, rng)
    small = tuple(np.concatenate([a[:1500], b[:1500]]) for a, b in zip(aimed, rand))
    both = tuple(np.concatenate([a, b]) for a, b in zip(big, small))
    one = Concordance(parent, ntaxa=T, engine=engine)
    two = Concordance(parent, ntaxa=T, engine=engine)
    host = Concordance(parent, ntaxa=T)
    one.add_dev(*to_dev(*both))
    two.add_dev(*to_dev(*big))
    two.add_dev(*to_dev(*small))
    host.add(*both)
    r1, r2 = one.raw(), two.raw()
    np.testing.assert_array_equal(r1["edge_counts"], r2["edge_counts"])
    np.testing.assert_array_equal(r1["tip_counts"], r2["tip_counts"])
    assert r1["skipped"] == r2["skipped"]
    np.testing.assert_allclose(r1["edge_sums"], r2["edge_sums"], rtol=1e-12)
    assert_same(two, host)
    # reset, then the same adds: the integer counters repeat
    two.reset()
    assert two.raw()["edge_counts"][:, 1:].sum() == 0 and two.raw()["tip_counts"].sum() == 0
    two.add_dev(*to_dev(*small))
    two.add_dev(*to_dev(*big))
    r3 = two.raw()
    np.testing.assert_array_equal(r3["edge_counts"], r1["edge_counts"])
    np.testing.assert_array_equal(r3["tip_counts"], r1["tip_counts"])
    assert r3["skipped"] == r1["skipped"]
    one.close()
    two.close()


@pytest.mark.parametrize("T", [256, 2052])
def test_small_row_counts_at_size(engine, T):
    """1 to 4 097 rows against the host: random rows, and aimed rows that all count.  At T = 2 052 the aimed rows
    start with those of edge 2 048, the only edge of the second pass (n = 1: that pass sees one row)."""
    from concordance_split_model import library_order
    from tetrad_amd.concordance import Concordance
    parent, model, aimed, rand, _ = big_case(T, "binary")
    rng = np.random.default_rng([T, 4])
    host = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25)
    dev = Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25, engine=engine)
    last = int(np.flatnonzero(library_order(host, model.masks) == host.n_edges - 1)[0])
    first = np.arange(last * K_TARGET, (last + 1) * K_TARGET)             # the rows aimed at the library's last edge
    for n in (1, 63, 64, 65, 4097):
        rest = rng.permutation(np.setdiff1d(np.arange(len(aimed[0])), first))
        pick = np.resize(np.concatenate([first, rest]), n)              # T = 256 has 1 012 aimed rows: they repeat
        for r, all_count in ((tuple(x[pick] for x in aimed), True), (mixed_rows(T, n, rng), False)):
            dev.reset()
            host.reset()
            dev.add_dev(*to_dev(*r))
            host.add(*r)
            assert_same(dev, host)
            counted = dev.raw()["edge_counts"][:, 1:5].sum(1)
            if all_count:
                assert counted.sum() == n and counted[-1] >= min(n, K_TARGET)
    dev.close()
