#!/usr/bin/env python
"""Time the site-pattern class rows and the D test loop (tetrad_amd/patterns.py, csrc/patterns.hpp).

At the c3 shape (128 taxa x 50 000 SNPs, 1e6 ascending sets), in full and in subsample mode, medians of `reps` by HIP
events on the call's stream:
  1. `tq_scan_dev` alone (ordering + site scan into the count slab);
  2. `tq_patterns_dev` (the same scan followed by tq_pattern_class_kernel);
  3. their difference = the class kernel, and the bandwidth that makes of its 1 088 bytes per set;
  4. a `run_dstat` loop of 20 replicates on every test with outgroup 0 of a 24-taxon source (wall clock, replicates/s).

    python tools/patterns_bench.py [reps] [--out FILE]
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
    res = {}
    for name, sub in (("full", False), ("subsample", True)):
        scan = event_ms(torch, lambda: eng.scan_dev(d_sets.data_ptr(), Q, sub, cs), reps)
        both = event_ms(torch, lambda: eng.patterns_dev(d_sets.data_ptr(), Q, sub, d_classes.data_ptr(), cs), reps)
        cls = both - scan
        res[name] = dict(scan_ms=round(scan, 4), patterns_ms=round(both, 4), class_kernel_ms=round(cls, 4),
                         class_kernel_GBps=round(Q * 1088 / cls / 1e6, 1) if cls > 0 else None,
                         counted_sites=int(d_classes[:, 15].sum(dtype=torch.int64).item()))
    return res


def bench_loop(eng, reps, nboots=20):
    Tl, Sl = 24, 20_000
    tmparr, tmpmap = synth.simulate_tmparr(Tl, Sl, seed=5)
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)].copy()
    seqarr[tmparr > 3] = ord("N")
    spans = bootstrap.get_spans(tmpmap)
    tests = patterns.tests_with_outgroup(Tl, 0)
    out = {}
    for name, sub in (("full", False), ("subsample", True)):
        walls = []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            res = patterns.run_dstat(eng, tmparr, tmpmap, seqarr, spans, tests, nboots, subsample_snps=sub, seed=r)
            walls.append(time.perf_counter() - t0)
        w = float(np.median(walls[1:]))
        out[name] = dict(tests=len(tests), sets=len(tests) // 3, nboots=nboots, wall_ms=round(w * 1e3, 3),
                         replicates_per_s=round(nboots / w, 1), finite_Z=int(np.isfinite(res["Z"]).sum()))
    return out


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 7
    with QuartetEngine(0) as eng:
        res = dict(tool="patterns_bench", reps=reps, shape=dict(T=T, S=S, sets=Q), kernels=bench_kernels(eng, reps))
    with QuartetEngine(0) as eng:
        res["run_dstat"] = bench_loop(eng, reps)
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
