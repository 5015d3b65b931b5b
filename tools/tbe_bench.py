#!/usr/bin/env python
"""Time the transfer bootstrap accumulator (tetrad_amd/tbe.py, csrc/tbe.hpp): the host back end on one core against
the device path, both through `tq_tbe_add` on the same prepared block of parent arrays.

  host    wall clock of one `add` into a host accumulator (tree preparation + masks + distances), single thread;
  device  HIP events on the call's stream around one `add` (tree preparation on the host, staging, the mask kernel and
          `tq_tbe_kernel` of all chunks, the waits between chunks included), and wall clock from the start of that add to
          the end of `read`.

Replicates are nearest-neighbour interchanges of one random tree; the reference is that tree.  The work is counted as
E x M x W x R word operations (one xor + popcount of a u64 word each; M = T - 2 nodes of a binary replicate).
Every leg: one warm-up, then the median of `runs` runs, each on a reset accumulator.  `--host-runs N` gives the host leg
fewer runs than the device leg (1 = a single run without warm-up: the host leg of the largest shape takes minutes);
`--host-only` needs no device.  The two back ends are asserted equal.

    python tools/tbe_bench.py [--runs 7] [--host-runs N] [--host-only] [T:R ...]
Prints one JSON line."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from consensus_bench import base_tree, nni  # noqa: E402  (tools/ is on the path of a script started from it)
from tetrad_amd.tbe import TransferSupport  # noqa: E402

SHAPES = [(128, 1000), (1024, 1000), (4096, 100)]


def tree_block(T, R, seed):
    """(the base tree, R trees each the base after 0..3 interchanges of its own, i32 [R, 2T - 1])."""
    rng = np.random.default_rng(seed)
    base = base_tree(T, rng)
    block = np.empty((R, 2 * T - 1), np.int32)
    for r in range(R):
        t = base
        for _ in range(int(rng.integers(0, 4))):
            t = nni(t, T, rng)
        block[r] = t
    return base, block


def add(acc, block, n_nodes, stream=None):
    rc = acc._lib.tq_tbe_add(acc._h, block.ctypes.data, n_nodes.ctypes.data, block.shape[0], block.shape[1], stream, None)
    acc._check(rc)


def timed(runs, fn):
    """ms of `runs` calls after one warm-up (no warm-up for a single run)."""
    out = []
    for i in range(runs + (runs > 1)):
        out.append(fn())
    return out[runs > 1:]


def time_shape(eng, T, R, runs, host_runs):
    ref, block = tree_block(T, R, seed=T + R)
    n_nodes = np.full(R, block.shape[1], np.int64)
    W = (T + 63) // 64
    res = dict(T=T, R=R, W=W)
    with TransferSupport(T, ref) as host:
        def host_run():
            host.reset()
            t0 = time.perf_counter()
            add(host, block, n_nodes)
            return (time.perf_counter() - t0) * 1e3
        ms = timed(host_runs, host_run)
        want = host.raw()
        E = len(want[1])
        ops = E * (T - 2) * W * R
        res.update(E=E, word_ops=ops, host_runs=host_runs, host_ms_median=float(np.median(ms)), host_ms_min=float(np.min(ms)),
                   host_gops=ops / (float(np.median(ms)) * 1e6))
    if eng is None:
        return res
    import torch
    with TransferSupport(T, ref, engine=eng) as dev:
        s = torch.cuda.current_stream()
        got = [None]

        def dev_run():
            dev.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            add(dev, block, n_nodes, ctypes.c_void_p(s.cuda_stream))
            e1.record(s)
            got[0] = dev.raw()
            wall = (time.perf_counter() - t0) * 1e3
            e1.synchronize()
            return e0.elapsed_time(e1), wall
        both = timed(runs, dev_run)
        ev, wall = [b[0] for b in both], [b[1] for b in both]
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want)), "device and host sums differ"
        st = dev.stats()
        res.update(dev_runs=runs, dev_event_ms_median=float(np.median(ev)), dev_event_ms_min=float(np.min(ev)),
                   dev_wall_to_read_ms_median=float(np.median(wall)), dev_wall_to_read_ms_min=float(np.min(wall)),
                   dev_gops=ops / (float(np.median(ev)) * 1e6), chunks=st["chunks"], chunk_trees=st["chunk_trees"],
                   host_over_device=res["host_ms_median"] / float(np.median(ev)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    host_runs = a.runs if a.host_runs is None else max(1, a.host_runs)
    if a.host_only:
        out = dict(shapes=[time_shape(None, T, R, a.runs, host_runs) for T, R in shapes], runs=a.runs, device=None)
    else:
        import torch
        from tetrad_amd.engine import QuartetEngine
        with QuartetEngine(0) as eng:
            out = dict(shapes=[time_shape(eng, T, R, a.runs, host_runs) for T, R in shapes], runs=a.runs,
                       device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
