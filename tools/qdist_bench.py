#!/usr/bin/env python
"""Time the quartet distance accumulator (tetrad_amd/qdist.py, csrc/qdist.hpp): the host back end on one core against
the device path, both through `tq_qd_add` + `tq_qd_score_ranks` on the same prepared block of parent arrays and the same
quartets.

  host    wall clock of one `add` (tree preparation, depth tables) + `score` (planes of every tree, N (N + 1) / 2 row
          products per chunk of 65 536 quartets) + `read` into a host accumulator, single thread;
  device  HIP events on the call's stream around `add` (tree preparation on the host, the upload, `tq_fit_table_kernel`),
          around `score` (rank upload or none, `tq_unrank_kernel`, `tq_qd_encode_kernel`, `tq_qd_gemm_kernel` per chunk)
          and around `read` (`tq_qd_final_kernel`, the copy of the two matrices), and the wall clock over all three.

Tree sets: every tree is one random binary tree after 0..3 nearest-neighbour interchanges of its own.  Quartets: `Q`
distinct sampled ranks (ascending), or all C(T, 4) as one range when Q is "all".  The product's work is counted as tile
pairs x 64 x 64 x plane words: the word-triples (`qd_word`: four u64 and + popcount) the kernel executes, padding rows
included; printed per second of the score interval beside the 2.1e12 word operations per second that profiles/tbe/ records
for `tq_tbe_kernel` (context only: that is one and + popcount per word over a whole add, this is four over an interval that
also holds the encode kernel).
Every leg: one warm-up, then the median of `runs` runs, each on a reset accumulator.  `--host-runs N` gives the host leg
fewer runs (1 = a single run without warm-up); `--host-only` needs no device; `--device-only` skips the host leg and the
comparison (for a run under a profiler); `--no-ab` skips the A/B.  The two back ends are asserted equal.
The first shape is also scored with the option `qdist_kslices` = 1 against auto (A/B of the k split, score interval).

    python tools/qdist_bench.py [--runs 7] [--host-runs N] [--host-only | --device-only] [--no-ab] [T:N:Q ...]
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

from consensus_bench import base_tree, nni  # noqa: E402  (tools/ is on the path of a script started from it)
from tetrad_amd.qdist import QuartetDistances  # noqa: E402

SHAPES = [(128, 1000, 10 ** 6), (128, 200, "all"), (1024, 200, 10 ** 6)]
TBE_WORD_OPS_PER_S = 2.1e12


def tree_block(T, N, seed):
    rng = np.random.default_rng(seed)
    base = base_tree(T, rng)
    block = np.empty((N, 2 * T - 1), np.int32)
    for r in range(N):
        t = base
        for _ in range(int(rng.integers(0, 4))):
            t = nni(t, T, rng)
        block[r] = t
    return block


def add(acc, block, n_nodes, stream=None):
    acc._check(acc._lib.tq_qd_add(acc._h, block.ctypes.data, n_nodes.ctypes.data, block.shape[0], block.shape[1], stream))


def score(acc, ranks, total, stream=None):
    if ranks is None:
        acc._check(acc._lib.tq_qd_score_ranks(acc._h, None, 0, total, stream))
    else:
        acc._check(acc._lib.tq_qd_score_ranks(acc._h, ranks.ctypes.data, 0, len(ranks), stream))


def timed(runs, fn):
    """results of `runs` calls after one warm-up (no warm-up for a single run)."""
    out = []
    for i in range(runs + (runs > 1)):
        out.append(fn())
        print(f"  run {i}: {out[-1]}", file=sys.stderr, flush=True)
    return out[runs > 1:]


def device_leg(eng, T, N, block, n_nodes, ranks, Q, runs, want):
    import torch
    with QuartetDistances(T, N, engine=eng) as dev:
        s = torch.cuda.current_stream()
        sp = ctypes.c_void_p(s.cuda_stream)
        got = [None]

        def dev_run():
            dev.reset()
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            t0 = time.perf_counter()
            e[0].record(s)
            add(dev, block, n_nodes, sp)
            e[1].record(s)
            score(dev, ranks, Q, sp)
            e[2].record(s)
            got[0] = dev.raw()
            e[3].record(s)
            e[3].synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]), wall
        rows = timed(runs, dev_run)
        if want is not None:
            assert all(np.array_equal(a, b) for a, b in zip(got[0], want)), "device and host matrices differ"
        med = [float(np.median([r[i] for r in rows])) for i in range(4)]
        return med, float(np.min([r[3] for r in rows])), dev.stats(), got[0]


def time_shape(eng, T, N, Q, runs, host_runs, ab):
    total = comb(T, 4)
    block = tree_block(T, N, seed=T + N)
    n_nodes = np.full(N, block.shape[1], np.int64)
    if Q == "all":
        ranks, Q = None, total
    else:
        ranks = np.sort(np.random.default_rng(T + N).choice(total, size=Q, replace=False)).astype(np.uint64)
    words, nt = -(-Q // 64), -(-N // 64)
    triples = nt * (nt + 1) // 2 * 64 * 64 * words
    res = dict(T=T, N=N, Q=Q, sampled=ranks is not None, plane_words=words, gemm_word_triples=triples,
               table_lookups=N * Q * 6)
    want = [None]
    print(f"shape T={T} N={N} Q={Q}: host", file=sys.stderr, flush=True)
    with QuartetDistances(T, N) as host:
        if host_runs == 0:                                          # --device-only: nothing to compare with
            host = None

        def host_run():
            host.reset()
            t0 = time.perf_counter()
            add(host, block, n_nodes)
            t1 = time.perf_counter()
            score(host, ranks, Q)
            want[0] = host.raw()
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3
        rows = timed(host_runs, host_run) if host is not None else []
        tot = [a + b for a, b in rows]
        if rows:
            res.update(host_runs=host_runs, host_add_ms_median=float(np.median([r[0] for r in rows])),
                       host_score_ms_median=float(np.median([r[1] for r in rows])), host_ms_median=float(np.median(tot)),
                       host_ms_min=float(np.min(tot)), mean_distance=host.mean_distance(),
                       mean_resolved=float(host.resolved().mean()))
    if eng is None:
        return res
    print(f"shape T={T} N={N} Q={Q}: device", file=sys.stderr, flush=True)
    med, wall_min, st, _ = device_leg(eng, T, N, block, n_nodes, ranks, Q, runs, want[0])
    add_ms, score_ms, read_ms, wall = med
    res.update(dev_runs=runs, dev_add_event_ms_median=add_ms, dev_score_event_ms_median=score_ms,
               dev_read_event_ms_median=read_ms, dev_total_event_ms_median=add_ms + score_ms + read_ms,
               dev_wall_ms_median=wall, dev_wall_ms_min=wall_min,
               word_triples_per_s_over_score=triples / (score_ms * 1e-3) if score_ms > 0 else None,
               tbe_word_ops_per_s_context=TBE_WORD_OPS_PER_S, kslices=st["kslices"], chunks_per_run=st["chunks"],
               chunk_quartets=st["chunk_quartets"], table_form=st["table_form"],
               host_over_device=res["host_ms_median"] / wall if "host_ms_median" in res else None)
    if ab:
        print("A/B qdist_kslices = 1", file=sys.stderr, flush=True)
        eng.set_option("qdist_kslices", 1)
        try:
            med1, _, st1, _ = device_leg(eng, T, N, block, n_nodes, ranks, Q, runs, want[0])
        finally:
            eng.set_option("qdist_kslices", 0)
        res.update(ab_kslices_1_score_event_ms_median=med1[1], ab_kslices_1_used=st1["kslices"],
                   ab_auto_score_event_ms_median=score_ms, ab_auto_used=st["kslices"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=None)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-ab", action="store_true")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = [(int(s.split(":")[0]), int(s.split(":")[1]), s.split(":")[2]) for s in a.shapes] or SHAPES
    shapes = [(T, N, Q if Q == "all" else int(Q)) for T, N, Q in shapes]
    host_runs = 0 if a.device_only else a.runs if a.host_runs is None else max(1, a.host_runs)
    if a.host_only:
        out = dict(shapes=[time_shape(None, T, N, Q, a.runs, host_runs, False) for T, N, Q in shapes], runs=a.runs, device=None)
    else:
        import torch
        from tetrad_amd.engine import QuartetEngine
        with QuartetEngine(0) as eng:
            out = dict(shapes=[time_shape(eng, T, N, Q, a.runs, host_runs, i == 0 and not a.no_ab) for i, (T, N, Q) in enumerate(shapes)],
                       runs=a.runs, device=torch.cuda.get_device_name(0), num_cu=eng.device_info()["num_cu"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
