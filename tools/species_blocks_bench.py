#!/usr/bin/env python
"""Time the pooled block rows of species sets (tetrad_amd/csrc/species_blocks.hpp).

Two shapes, both 128 samples x 50 000 sites with all C(K,4) species sets: K = 32 species x 4 lineages and K = 64 x 2.
Medians of `reps` by HIP events on the call's stream, all in one run:
  1. `tq_patterns_species_dev` (pooling kernel + class kernel: what a replicate of `run_dstat(species_of=...)` pays,
     without its build), comparable with the block form at B = 1;
  2. `tq_patterns_blocks_species_dev` at B = 1, 20 and 50 equal blocks (rows in chunks of sets that keep the output
     below 1 GiB, the chunks' times summed); at B = 1 the tool asserts the rows equal those of 1.;
  3. the other way to get such rows today: the n^4 lineage quartets of a 1 000-set sample through
     `tq_patterns_blocks_dev` at the same B, scaled up to all sets (the sum over the quartets not included);
  4. wall clock of `run_dstat(nboots=20, species_of=...)` against `run_dstat_jackknife(nblocks=50, species_of=...)` on
     every test with outgroup species 0 of the K = 32 shape.

    python tools/species_blocks_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
import time
from itertools import combinations, product
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import bootstrap, patterns, synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

S = 50_000
SHAPES = ((32, 4), (64, 2))
OUT_BYTES = 1 << 30
SAMPLE = 1000


def event_ms(torch, fn, reps):
    fn()                                                            # warm-up: allocations, first launch, the species table
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


def bench_shape(eng, K, n_per, reps):
    import torch
    tmparr, tmpmap, sp, _ = synth.simulate_species(K, n_per, S, seed=100 + K)
    eng.set_data(tmparr, tmpmap)
    eng.set_species(sp, K)
    ssets = np.array(list(combinations(range(K), 4)), np.uint32)
    Q = len(ssets)
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_classes = torch.empty((Q, 16), dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    res = dict(K=K, lineages=n_per, sets=Q)
    res["patterns_species_ms"] = round(event_ms(torch, lambda: eng.patterns_species_dev(d_sets.data_ptr(), Q,
                                                                                       d_classes.data_ptr(), cs), reps), 4)
    # the lineage quartets of a sample of the sets, in role order
    rng = np.random.default_rng(K)
    pick = np.sort(rng.choice(Q, size=min(SAMPLE, Q), replace=False))
    mem = [np.flatnonzero(sp == k) for k in range(K)]
    lin = np.array([q for s in ssets[pick] for q in product(*(mem[int(k)] for k in s))], np.uint32)
    d_lin = torch.from_numpy(lin.view(np.int32)).cuda()
    res["expansion_sample_sets"], res["expansion_quartets"] = len(pick), len(lin)
    for B in (1, 20, 50):
        starts = np.linspace(0, S, B + 1).astype(np.int64)
        chunk = min(Q, OUT_BYTES // (B * 64))
        d_rows = torch.empty((chunk, B, 16), dtype=torch.int32, device="cuda")

        def rows():
            for q0 in range(0, Q, chunk):
                eng.patterns_blocks_species_dev(d_sets.data_ptr() + 16 * q0, min(chunk, Q - q0), starts, d_rows.data_ptr(), cs)

        res[f"blocks_species_B{B}_ms"] = round(event_ms(torch, rows, reps), 4)
        if B == 1:                                                  # the same rows as the pooling path
            assert chunk == Q and torch.equal(d_rows[:, 0], d_classes)
        del d_rows
        d_lrows = torch.empty((len(lin), B, 16), dtype=torch.int32, device="cuda")
        ms = event_ms(torch, lambda: eng.patterns_blocks_dev(d_lin.data_ptr(), len(lin), starts, d_lrows.data_ptr(), cs), reps)
        res[f"expansion_B{B}_sample_ms"] = round(ms, 4)
        res[f"expansion_B{B}_scaled_ms"] = round(ms * Q / len(pick), 3)
        del d_lrows
    return res, (tmparr, tmpmap, sp)


def bench_loop(eng, data, K, reps, nboots=20, nblocks=50):
    tmparr, tmpmap, sp = data
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)].copy()
    seqarr[tmparr > 3] = ord("N")
    spans = bootstrap.get_spans(tmpmap)
    tests = patterns.tests_with_outgroup(K, 0)
    boot, jack = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        rb = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, spans, tests, nboots, seed=r, species_of=sp)
        t1 = time.perf_counter()
        rj = patterns.run_dstat_jackknife(eng, tmparr, tmpmap, tests, nblocks=nblocks, species_of=sp)
        t2 = time.perf_counter()
        boot.append(t1 - t0)
        jack.append(t2 - t1)
    assert np.array_equal(rb["abba"], rj["abba"]) and np.array_equal(rb["baba"], rj["baba"])
    ok = np.isfinite(rb["Z"]) & np.isfinite(rj["Z"])
    return dict(K=K, tests=len(tests), sets=len(tests) // 3, nboots=nboots, nblocks=nblocks,
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
    res = dict(tool="species_blocks_bench", reps=reps, S=S, shapes=[])
    loop_data = None
    for K, n_per in SHAPES:
        with QuartetEngine(0) as eng:
            r, data = bench_shape(eng, K, n_per, reps)
        res["shapes"].append(r)
        if loop_data is None:
            loop_data = (data, K)
    with QuartetEngine(0) as eng:
        res["dstat"] = bench_loop(eng, loop_data[0], loop_data[1], reps)
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
