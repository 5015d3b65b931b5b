#!/usr/bin/env python
"""Time the consensus accumulator (tetrad_amd/consensus.py, csrc/consensus.hpp): the host back end on one core against
the device path, both through `tq_cons_add` on the same prepared block of parent arrays.

  host    wall clock of one `add` into a host accumulator (tree preparation + masks + exact map), single thread;
  device  HIP events around one `add` (tree preparation on the host, staging, the mask / insert / count kernels of all
          chunks but the waits between chunks included), and wall clock from the start of that add to the end of `read`.

Trees are random nearest-neighbour interchanges of one random tree, so the table stays near 2 T distinct splits.
Every leg: one warm-up, then the median of `runs` (>= 5) runs, each on a reset accumulator.

    python tools/consensus_bench.py [runs] [T:R ...]
Prints one JSON line."""
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tetrad_amd import synth  # noqa: E402
from tetrad_amd.consensus import Consensus  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

SHAPES = [(128, 100), (128, 1000), (1024, 1000), (4096, 200)]


def base_tree(T, rng):
    children, root = synth.random_tree_children(T, rng)
    parent = np.full(2 * T - 1, -1, np.int32)
    for v, (a, b) in children.items():
        parent[a] = parent[b] = v
    return parent


def nni(parent, T, rng):
    """One nearest-neighbour interchange over a random internal edge of a binary tree."""
    parent = parent.copy()
    while True:
        v = int(rng.integers(T, len(parent)))
        u = int(parent[v])
        if u < 0:
            continue
        kids = np.flatnonzero(parent == v)
        sibs = np.flatnonzero(parent == u)
        sibs = sibs[sibs != v]
        c, s = int(rng.choice(kids)), int(rng.choice(sibs))
        parent[c], parent[s] = u, v
        return parent


def tree_block(T, R, seed):
    """R trees, each the base tree after 0..3 interchanges of its own (i32 [R, 2T - 1])."""
    rng = np.random.default_rng(seed)
    base = base_tree(T, rng)
    block = np.empty((R, 2 * T - 1), np.int32)
    for r in range(R):
        t = base
        for _ in range(int(rng.integers(0, 4))):
            t = nni(t, T, rng)
        block[r] = t
    return block


def add(acc, block, n_nodes, stream=None):
    rc = acc._lib.tq_cons_add(acc._h, block.ctypes.data, n_nodes.ctypes.data, block.shape[0], block.shape[1], stream)
    acc._check(rc)


def time_shape(eng, T, R, runs):
    block = tree_block(T, R, seed=T + R)
    n_nodes = np.full(R, block.shape[1], np.int64)
    max_splits = 64 * T
    res = dict(T=T, R=R, TR=T * R)
    with Consensus(T, max_splits) as host:
        ms = []
        for i in range(runs + 1):
            host.reset()
            t0 = time.perf_counter()
            add(host, block, n_nodes)
            ms.append((time.perf_counter() - t0) * 1e3)
        want = host.raw()
        res.update(host_ms_median=float(np.median(ms[1:])), host_ms_min=float(np.min(ms[1:])), splits=int(len(want[1])))
    with Consensus(T, max_splits, engine=eng) as dev:
        s = torch.cuda.current_stream()
        ev, wall = [], []
        for i in range(runs + 1):
            dev.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            add(dev, block, n_nodes, ctypes.c_void_p(s.cuda_stream))
            e1.record(s)
            got = dev.raw()
            wall.append((time.perf_counter() - t0) * 1e3)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "device and host tables differ"
        st = dev.stats()
        res.update(dev_event_ms_median=float(np.median(ev[1:])), dev_event_ms_min=float(np.min(ev[1:])),
                   dev_wall_to_read_ms_median=float(np.median(wall[1:])), dev_wall_to_read_ms_min=float(np.min(wall[1:])),
                   chunks=st["chunks"], chunk_trees=st["chunk_trees"], unresolved=st["unresolved"])
    res["device_faster"] = res["dev_wall_to_read_ms_median"] < res["host_ms_median"]
    return res


def main():
    runs = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    shapes = [tuple(int(x) for x in a.split(":")) for a in sys.argv[2:]] or SHAPES
    with QuartetEngine(0) as eng:
        out = dict(shapes=[time_shape(eng, T, R, runs) for T, R in shapes], runs=runs, device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
