#!/usr/bin/env python
"""Time the tree distance accumulator (tetrad_amd/treedist.py, csrc/treedist.hpp): the host back end on one core against
the device path, both through `tq_rf_add` + `tq_rf_read` on the same prepared block of parent arrays.

  host    wall clock of one `add` + `read` into a host accumulator (tree preparation, masks, the exact map, N (N - 1) / 2
          merges of id lists), single thread;
  device  HIP events on the call's stream around `add` (tree preparation on the host, staging, the mask, insert and ident
          kernels of all chunks, the waits between chunks included) and around `read` (columns on the host, scatter,
          `tq_rf_gemm_kernel`, epilogue, the copy of the three arrays), and wall clock over both.

Tree sets: "nni" = every tree is one random tree after 0..3 nearest-neighbour interchanges of its own; "random" = every
tree is a random tree of its own (unrelated: few splits are shared by chance, but every shared one is a column of its
own).  The product's work is counted as tile pairs x 64 x 64 x column words: the u64 and + popcount steps the kernel
executes, padding rows included.
Every leg: one warm-up, then the median of `runs` runs, each on a reset accumulator.  `--host-runs N` gives the host leg
fewer runs than the device leg (1 = a single run without warm-up); `--host-only` needs no device.  The two back ends are
asserted equal.

    python tools/treedist_bench.py [--runs 7] [--host-runs N] [--host-only] [T:N:kind ...]
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
from tetrad_amd.treedist import TreeDistances  # noqa: E402

SHAPES = [(128, 1000, "nni"), (1024, 1000, "nni"), (4096, 200, "nni"), (1024, 1000, "random")]


def tree_block(T, N, kind, seed):
    rng = np.random.default_rng(seed)
    base = base_tree(T, rng)
    block = np.empty((N, 2 * T - 1), np.int32)
    for r in range(N):
        if kind == "random":
            block[r] = base_tree(T, rng)
            continue
        t = base
        for _ in range(int(rng.integers(0, 4))):
            t = nni(t, T, rng)
        block[r] = t
    return block


def add(acc, block, n_nodes, stream=None):
    acc._check(acc._lib.tq_rf_add(acc._h, block.ctypes.data, n_nodes.ctypes.data, block.shape[0], block.shape[1], stream))


def timed(runs, fn):
    """results of `runs` calls after one warm-up (no warm-up for a single run)."""
    out = []
    for i in range(runs + (runs > 1)):
        out.append(fn())
    return out[runs > 1:]


def time_shape(eng, T, N, kind, runs, host_runs):
    block = tree_block(T, N, kind, seed=T + N)
    n_nodes = np.full(N, block.shape[1], np.int64)
    res = dict(T=T, N=N, kind=kind, W=(T + 63) // 64)
    with TreeDistances(T, N) as host:
        want = [None]

        def host_run():
            host.reset()
            t0 = time.perf_counter()
            add(host, block, n_nodes)
            want[0] = host.raw()
            return (time.perf_counter() - t0) * 1e3
        ms = timed(host_runs, host_run)
        columns = host.stats()["columns"]
        nt, cw = -(-N // 64), -(-columns // 64)
        ops = nt * (nt + 1) // 2 * 64 * 64 * cw
        res.update(columns=columns, column_words=cw, distinct_splits=host.ndistinct, gemm_word_ops=ops, host_runs=host_runs,
                   host_ms_median=float(np.median(ms)), host_ms_min=float(np.min(ms)), mean_rf=host.mean_rf())
    if eng is None:
        return res
    import torch
    with TreeDistances(T, N, engine=eng) as dev:
        s = torch.cuda.current_stream()
        got = [None]

        def dev_run():
            dev.reset()
            torch.cuda.synchronize()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            t0 = time.perf_counter()
            e0.record(s)
            add(dev, block, n_nodes, ctypes.c_void_p(s.cuda_stream))
            e1.record(s)
            got[0] = dev.raw()
            e2.record(s)
            e2.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            return e0.elapsed_time(e1), e1.elapsed_time(e2), wall
        rows = timed(runs, dev_run)
        add_ms, read_ms, wall = (float(np.median([r[i] for r in rows])) for i in range(3))
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])), "device and host arrays differ"
        st = dev.stats()
        assert st["columns"] == columns
        res.update(dev_runs=runs, dev_add_event_ms_median=add_ms, dev_read_event_ms_median=read_ms,
                   dev_total_event_ms_median=add_ms + read_ms, dev_wall_ms_median=wall,
                   dev_wall_ms_min=float(np.min([r[2] for r in rows])),
                   gemm_word_ops_per_s_over_read=ops / (read_ms * 1e-3) if read_ms > 0 else None,
                   chunks=st["chunks"], chunk_trees=st["chunk_trees"], col_chunks=st["col_chunks"],
                   col_words_chunk=st["col_words_chunk"], host_over_device=res["host_ms_median"] / wall)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = [(int(s.split(":")[0]), int(s.split(":")[1]), s.split(":")[2]) for s in a.shapes] or SHAPES
    host_runs = a.runs if a.host_runs is None else max(1, a.host_runs)
    if a.host_only:
        out = dict(shapes=[time_shape(None, T, N, k, a.runs, host_runs) for T, N, k in shapes], runs=a.runs, device=None)
    else:
        import torch
        from tetrad_amd.engine import QuartetEngine
        with QuartetEngine(0) as eng:
            out = dict(shapes=[time_shape(eng, T, N, k, a.runs, host_runs) for T, N, k in shapes], runs=a.runs,
                       device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
