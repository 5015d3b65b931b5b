#!/usr/bin/env python
"""Time the per-block class rows and the block jackknife (tetrad_amd/patterns.py, csrc/pattern_blocks.hpp).

At the c3 shape (128 taxa x 50 000 SNPs, 1e6 ascending sets), full mode, medians of `reps` by HIP events on the call's
stream, all in one run:
  1. `tq_patterns_dev` (the histogram scan followed by the class kernel: what a replicate of `run_dstat` pays);
  2. `tq_patterns_blocks_dev` at B = 1, 20 and 50 equal blocks (rows in chunks of sets that keep the output below
     1 GiB, the chunks' times summed);
  3. `tq_dstat_jackknife_dev` at B = 50 on three tests per set of one such chunk, scaled to 3e6 tests;
  4. wall clock of `run_dstat` with 20 replicates against `run_dstat_jackknife` with 50 blocks on every test with
     outgroup 0 of a 24-taxon x 20 000-site source (the case of tools/patterns_bench.py).

    python tools/blocks_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import bootstrap, patterns, synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

T, S, Q = 128, 50_000, 1_000_000
OUT_BYTES = 1 << 30


def event_ms(torch, fn, reps):
    fn()                                                            # warm-up: allocations, first launch
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def bench_kernels(eng, reps):
    import torch
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    eng.set_data(tmparr, tmpmap)
    sets = np.sort(synth.random_quartets(T, Q, seed=7).astype(np.uint32), axis=1)
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    d_classes = torch.empty((Q, 16), dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    res = dict(patterns_ms=round(event_ms(torch, lambda: eng.patterns_dev(d_sets.data_ptr(), Q, False, d_classes.data_ptr(),
                                                                          cs), reps), 4))
    whole = d_classes[:, 15].sum(dtype=torch.int64).item()
    for B in (1, 20, 50):
        starts = np.linspace(0, S, B + 1).astype(np.int64)
        chunk = min(Q, OUT_BYTES // (B * 64))
        d_rows = torch.empty((chunk, B, 16), dtype=torch.int32, device="cuda")

        def rows():
            for q0 in range(0, Q, chunk):
                eng.patterns_blocks_dev(d_sets.data_ptr() + 16 * q0, min(chunk, Q - q0), starts, d_rows.data_ptr(), cs)

        res[f"blocks_B{B}_ms"] = round(event_ms(torch, rows, reps), 4)
        if B == 1:                                                  # the same counts as the histogram scan
            assert d_rows[:, 0, 15].sum(dtype=torch.int64).item() == whole
        if B == 50:
            n_sets = min(chunk, Q - (Q - 1) // chunk * chunk)       # the chunk the last call left in d_rows
            N = 3 * n_sets
            d_set_of = torch.from_numpy(np.repeat(np.arange(n_sets, dtype=np.int32), 3)).cuda()
            d_ia = torch.from_numpy(np.tile(np.array([8, 6, 3], np.uint8), n_sets)).cuda()
            d_ib = torch.from_numpy(np.tile(np.array([6, 3, 8], np.uint8), n_sets)).cuda()
            d_out = torch.empty((N, 4), dtype=torch.float64, device="cuda")
            ms = event_ms(torch, lambda: eng.dstat_jackknife_dev(d_rows.data_ptr(), n_sets, B, d_set_of.data_ptr(),
                                                                 d_ia.data_ptr(), d_ib.data_ptr(), N, d_out.data_ptr(), cs), reps)
            res["jackknife_B50_tests"] = N
            res["jackknife_B50_ms"] = round(ms, 4)
            res["jackknife_B50_ms_per_3e6_tests"] = round(ms * 3 * Q / N, 4)
        del d_rows
    return res


def bench_loop(eng, reps, nboots=20, nblocks=50):
    Tl, Sl = 24, 20_000
    tmparr, tmpmap = synth.simulate_tmparr(Tl, Sl, seed=5)
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)].copy()
    seqarr[tmparr > 3] = ord("N")
    spans = bootstrap.get_spans(tmpmap)
    tests = patterns.tests_with_outgroup(Tl, 0)
    boot, jack = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        rb = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, spans, tests, nboots, seed=r)
        t1 = time.perf_counter()
        rj = patterns.run_dstat_jackknife(eng, tmparr, tmpmap, tests, nblocks=nblocks)
        t2 = time.perf_counter()
        boot.append(t1 - t0)
        jack.append(t2 - t1)
    ok = np.isfinite(rb["Z"]) & np.isfinite(rj["Z"])
    return dict(tests=len(tests), sets=len(tests) // 3, nboots=nboots, nblocks=nblocks,
                run_dstat_wall_ms=round(float(np.median(boot[1:])) * 1e3, 3),
                run_dstat_jackknife_wall_ms=round(float(np.median(jack[1:])) * 1e3, 3),
                finite_Z_both=int(ok.sum()),
                median_se_ratio_jackknife_over_bootstrap=round(float(np.median(rj["jk_se"][ok] / rb["boot_std"][ok])), 4))


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 7
    with QuartetEngine(0) as eng:
        res = dict(tool="blocks_bench", reps=reps, shape=dict(T=T, S=S, sets=Q), kernels=bench_kernels(eng, reps))
    with QuartetEngine(0) as eng:
        res["dstat"] = bench_loop(eng, reps)
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
