"""GPU: the concordance kernel (`tq_conc_add_dev`) equals the host accumulator on the same rows -- integer counters
bit-exact, the weight / score sums within 1e-12 relative -- on the LDS-table path (T = 128) and the global-table path
(T = 600); the replicate loop feeds it every replicate's rows; two ranks reduce to one."""
import ctypes
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from concordance_model import random_tree

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
