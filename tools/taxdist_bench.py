#!/usr/bin/env python
"""Time the taxon counts (tetrad_amd/distance.py, csrc/taxdist.hpp): the device path on the resident replicate against
the host execution on the u8 matrix, and the sweep of the work-item length.

  device  HIP events on the call's stream around `taxon_counts_dev` into a device buffer (the zeroing of the rows, the
          upload of the work items, `tq_taxon_counts_kernel`, `tq_taxon_finish_kernel`; asynchronous): one warm-up, then
          the median of `runs` runs; and the wall clock of the synchronous `taxon_counts` (with the copy of the rows back).
  sweep   the same events with option "taxdist_slice_words" = 8, 16, 32, 64, 128.
  host    one run of `taxon_counts_host` on one core by the wall clock (packing the matrix into words included).
The two back ends are asserted equal.  The word-rule rate is pairs x words / time with pairs = T (T + 1) / 2 and words =
the u64 words of the blocks: the rule applications a perfect triangle needs (the diagonal tiles compute both halves).

    python tools/taxdist_bench.py [--runs 7] [--no-host] [--no-sweep] [T:S:B ...]
Shapes default to 128:50000:1, 128:50000:50 (the matrix of config c3) and 1024:200000:1 (`simulate_tmparr`).
Prints one JSON line (progress goes to stderr)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tetrad_amd import distance, synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

SHAPES = [(128, 50_000, 1), (128, 50_000, 50), (1024, 200_000, 1)]
SLICES = (8, 16, 32, 64, 128)
_MATRIX = {}


def matrix(T, S):
    if (T, S) not in _MATRIX:
        _MATRIX.clear()
        c3 = synth.CONFIGS["c3"][:2] == (T, S)                     # the matrix of config c3 itself where the shape is its
        _MATRIX[T, S] = synth.simulate_tmparr(T, S, seed=synth.CONFIG_SEEDS["c3"] if c3 else 3)
    return _MATRIX[T, S]


def event_ms(eng, starts, d_out, runs):
    import torch
    s = torch.cuda.current_stream()
    times = []
    for i in range(runs + 1):                                       # the first is the warm-up
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        eng.taxon_counts_dev(starts, d_out.data_ptr(), s.cuda_stream)
        b.record(s)
        b.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def time_shape(eng, T, S, B, runs, host, sweep):
    import torch
    print(f"shape T={T} S={S} B={B}: data", file=sys.stderr, flush=True)
    tmparr, tmpmap = matrix(T, S)
    starts = np.linspace(0, S, B + 1).astype(np.int64)
    eng.set_data(tmparr, tmpmap)
    d_out = torch.empty((B, T, T, 4), dtype=torch.int32, device="cuda")
    words = int(sum((starts[j + 1] - 1) // 64 - starts[j] // 64 + 1 for j in range(B)))
    pair_words = T * (T + 1) // 2 * words
    res = dict(T=T, S=S, B=B, words=words, pair_words=pair_words, runs=runs)
    print(f"shape T={T} S={S} B={B}: device", file=sys.stderr, flush=True)
    med, low = event_ms(eng, starts, d_out, runs)
    st = eng.taxon_counts_stats()
    got = d_out.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    sync = eng.taxon_counts(starts)
    wall = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(sync, got), "the device form and the host-buffer form differ"
    res.update(dev_event_ms_median=med, dev_event_ms_min=low, dev_sync_wall_ms=wall, slice_words=st["slice_words"],
               work_items=st["work_items"], tile_pairs=st["tile_pairs"], workgroups=st["work_items"] * st["tile_pairs"],
               pair_words_per_s=pair_words / (med * 1e-3))
    if sweep:
        res["sweep"] = {}
        for w in SLICES:
            eng.set_option("taxdist_slice_words", w)
            m, lo = event_ms(eng, starts, d_out, runs)
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), got), f"slice length {w} changes the counts"
            res["sweep"][str(w)] = dict(event_ms_median=m, event_ms_min=lo, work_items=eng.taxon_counts_stats()["work_items"])
        eng.set_option("taxdist_slice_words", 0)
    if host:
        print(f"shape T={T} S={S} B={B}: host", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        want = distance.taxon_counts_host(tmparr, starts)
        res["host_wall_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(want, got), "device and host counts differ"
        res["host_over_device"] = res["host_wall_ms"] / med
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("shapes", nargs="*")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes] or SHAPES
    import torch
    with QuartetEngine(0) as eng:
        out = dict(shapes=[time_shape(eng, T, S, B, a.runs, not a.no_host, not a.no_sweep) for T, S, B in shapes],
                   device=torch.cuda.get_device_name(0), num_cu=eng.device_info()["num_cu"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
