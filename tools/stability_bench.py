#!/usr/bin/env python
"""Time the leaf stability accumulator (tetrad_amd/stability.py, csrc/stability.hpp): the host back end on one core
against the device path, both through `tq_ls_add` + `tq_ls_score_ranks` on the same prepared block of parent arrays and
the same quartets.

  host    wall clock of one `add` (tree preparation, depth tables) + `score` with a counts array (planes of every tree,
          then a loop over the bits of every quartet along the trees, per chunk of 65 536 quartets) + `read`, single thread;
  device  HIP events on the call's stream around `add` (tree preparation on the host, the upload, `tq_fit_table_kernel`),
          around `score` without a counts array (rank upload or none, `tq_unrank_kernel`, `tq_qd_encode_kernel`,
          `tq_ls_count_kernel` per chunk; asynchronous), around `read`, and -- on a cleared accumulator with the same
          trees -- around `score` with a counts array (the rows come back chunk by chunk; the call waits), and the wall
          clock over add + score + read.

Tree sets and quartets as tools/qdist_bench.py: every tree is one random binary tree after 0..3 nearest-neighbour
interchanges of its own; `Q` distinct sampled ranks (ascending), or all C(T, 4) as one range when Q is "all".  The count
kernel's work is counted as trees x 3 x plane words: the word visits (one LDS broadcast read, one shift, one and + add
per lane) it executes.
Every leg: one warm-up, then the median of `runs` runs, each on a reset accumulator.  `--host-runs N` gives the host leg
fewer runs (1 = a single run without warm-up); `--host-only` needs no device; `--device-only` skips the host leg and the
comparison (for a run under a profiler).  The two back ends are asserted equal, sums and counts both.

    python tools/stability_bench.py [--runs 7] [--host-runs N] [--host-only | --device-only] [T:N:Q ...]
Prints one JSON line (progress goes to stderr)."""
import argparse
import ctypes
import json
import sys
import time
from math import comb
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from qdist_bench import timed, tree_block  # noqa: E402  (tools/ is on the path of a script started from it)
from tetrad_amd.stability import LeafStability  # noqa: E402

SHAPES = [(128, 1000, 10 ** 6), (128, 200, "all")]


def add(acc, block, n_nodes, stream=None):
    acc._check(acc._lib.tq_ls_add(acc._h, block.ctypes.data, n_nodes.ctypes.data, block.shape[0], block.shape[1], stream))


def score(acc, ranks, total, counts=None, stream=None):
    table = None if counts is None else counts.ctypes.data
    if ranks is None:
        acc._check(acc._lib.tq_ls_score_ranks(acc._h, None, 0, total, table, stream))
    else:
        acc._check(acc._lib.tq_ls_score_ranks(acc._h, ranks.ctypes.data, 0, len(ranks), table, stream))


def device_leg(eng, T, N, block, n_nodes, ranks, Q, runs, want):
    import torch
    with LeafStability(T, N, engine=eng) as dev:
        s = torch.cuda.current_stream()
        sp = ctypes.c_void_p(s.cuda_stream)
        got = [None, np.zeros((Q, 4), np.uint16)]

        def dev_run():
            dev.reset()
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            t0 = time.perf_counter()
            e[0].record(s)
            add(dev, block, n_nodes, sp)
            e[1].record(s)
            score(dev, ranks, Q, None, sp)
            e[2].record(s)
            got[0] = dev.raw()
            e[3].record(s)
            e[3].synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            dev.clear()
            e[4].record(s)
            score(dev, ranks, Q, got[1], sp)
            e[5].record(s)
            e[5].synchronize()
            assert np.array_equal(dev.raw(), got[0]), "the sums with and without the counts array differ"
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), e[4].elapsed_time(e[5]), wall
        rows = timed(runs, dev_run)
        if want is not None:
            assert np.array_equal(got[0], want[0]), "device and host sums differ"
            assert np.array_equal(got[1], want[1]), "device and host counts differ"
        med = [float(np.median([r[i] for r in rows])) for i in range(5)]
        return med, float(np.min([r[4] for r in rows])), dev.stats(), dev.stability("dif")


def time_shape(eng, T, N, Q, runs, host_runs):
    total = comb(T, 4)
    block = tree_block(T, N, seed=T + N)
    n_nodes = np.full(N, block.shape[1], np.int64)
    if Q == "all":
        ranks, Q = None, total
    else:
        ranks = np.sort(np.random.default_rng(T + N).choice(total, size=Q, replace=False)).astype(np.uint64)
    words = -(-Q // 64)
    res = dict(T=T, N=N, Q=Q, sampled=ranks is not None, plane_words=words, count_word_visits=N * 3 * words,
               plane_bytes=N * 3 * words * 8, table_lookups=N * Q * 6)
    want = None
    print(f"shape T={T} N={N} Q={Q}: host", file=sys.stderr, flush=True)
    if host_runs:
        with LeafStability(T, N) as host:
            table = np.zeros((Q, 4), np.uint16)
            sums = [None]

            def host_run():
                host.reset()
                t0 = time.perf_counter()
                add(host, block, n_nodes)
                t1 = time.perf_counter()
                score(host, ranks, Q, table)
                sums[0] = host.raw()
                t2 = time.perf_counter()
                return (t1 - t0) * 1e3, (t2 - t1) * 1e3
            rows = timed(host_runs, host_run)
            want = (sums[0], table)
            tot = [a + b for a, b in rows]
            ls = host.stability("dif")
            res.update(host_runs=host_runs, host_add_ms_median=float(np.median([r[0] for r in rows])),
                       host_score_ms_median=float(np.median([r[1] for r in rows])), host_ms_median=float(np.median(tot)),
                       host_ms_min=float(np.min(tot)), ls_dif_min=float(ls.min()), ls_dif_max=float(ls.max()),
                       unresolved_share=float(table[:, 3].astype(np.int64).sum() / (N * Q)))
    if eng is None:
        return res
    print(f"shape T={T} N={N} Q={Q}: device", file=sys.stderr, flush=True)
    med, wall_min, st, _ = device_leg(eng, T, N, block, n_nodes, ranks, Q, runs, want)
    add_ms, score_ms, read_ms, score_counts_ms, wall = med
    res.update(dev_runs=runs, dev_add_event_ms_median=add_ms, dev_score_event_ms_median=score_ms,
               dev_read_event_ms_median=read_ms, dev_score_with_counts_event_ms_median=score_counts_ms,
               dev_total_event_ms_median=add_ms + score_ms + read_ms, dev_wall_ms_median=wall, dev_wall_ms_min=wall_min,
               chunks=st["chunks"], chunk_quartets=st["chunk_quartets"], table_form=st["table_form"],
               workgroups_last_launch=st["workgroups"], tree_tile=st["tree_tile"],
               host_over_device=res["host_ms_median"] / wall if "host_ms_median" in res else None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = [(int(s.split(":")[0]), int(s.split(":")[1]), s.split(":")[2]) for s in a.shapes] or SHAPES
    shapes = [(T, N, Q if Q == "all" else int(Q)) for T, N, Q in shapes]
    host_runs = 0 if a.device_only else a.runs if a.host_runs is None else max(1, a.host_runs)
    if a.host_only:
        out = dict(shapes=[time_shape(None, T, N, Q, a.runs, host_runs) for T, N, Q in shapes], runs=a.runs, device=None)
    else:
        import torch
        from tetrad_amd.engine import QuartetEngine
        with QuartetEngine(0) as eng:
            out = dict(shapes=[time_shape(eng, T, N, Q, a.runs, host_runs) for T, N, Q in shapes],
                       runs=a.runs, device=torch.cuda.get_device_name(0), num_cu=eng.device_info()["num_cu"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
