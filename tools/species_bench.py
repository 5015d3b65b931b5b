#!/usr/bin/env python
"""Time species mode (tetrad_amd/species.py, csrc/species.hpp) against the naive route.

For each shape (K species x n lineages, S = 50 000 sites, full mode, all C(K,4) species quartets):
  1. `resolve_species` with HIP-event timing, once per kernel form (option "species_method": MFMA, VALU): the species
     table build, the pooled-count kernel, the singular-value stage, and the wall time of the whole call (median of
     `reps`);
  2. the lower bound of the naive route: the engine's full-mode scan time (ordering + site scan, no singular values)
     of all expanded lineage quartets, K = 32 x 4 -> 9.2e6, K = 64 x 2 -> 1.0e7, resolved in batches.

    python tools/species_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
import time
from itertools import combinations
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

SHAPES = [(32, 4), (64, 2)]
S = 50_000


def bench_shape(eng, K, n, reps):
    T = K * n
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    rng = np.random.default_rng(K)
    sp = rng.permutation(np.repeat(np.arange(K, dtype=np.int32), n))
    eng.set_data(tmparr, tmpmap)
    eng.set_species(sp, K)
    rows = np.array(list(combinations(range(K), 4)), np.uint32)
    eng.timing_enable(True)
    forms = {}
    for name, method in (("mfma", 1), ("valu", 0)):
        eng.set_option("species_method", method)
        eng.resolve_species(rows)                                 # warm-up (builds the species table)
        eng.timing_read_kernels()
        walls, pool, svd = [], [], []
        for _ in range(reps):
            eng.set_data(tmparr, tmpmap)                          # the table is rebuilt on every call below
            eng.timing_read_kernels()
            t0 = time.perf_counter()
            rstat, _, flags = eng.resolve_species(rows)
            walls.append((time.perf_counter() - t0) * 1e3)
            k, _ = eng.timing_read_kernels()
            pool.append((k["order"], k["scan"]))
            svd.append(k["bidiag"] + k["bdsqr"] + k["score"])
        forms[name] = dict(table_ms=round(float(np.median([p[0] for p in pool])), 3),
                           pool_ms=round(float(np.median([p[1] for p in pool])), 3),
                           svd_ms=round(float(np.median(svd)), 3), call_ms=round(float(np.median(walls)), 3),
                           flagged_rows=int((flags != 0).sum()))
    eng.set_option("species_method", -1)
    # naive bound: full-mode scan of every lineage quartet
    mem = np.stack([np.flatnonzero(sp == k) for k in range(K)])      # [K, n]: every species has n lineages
    per = n ** 4
    total_lin = len(rows) * per
    step = max(1, (1 << 21) // per)
    eng.timing_read_split()
    scan_ms = 0.0
    for r0 in range(0, len(rows), step):
        r = rows[r0:r0 + step]
        g = np.broadcast_arrays(mem[r[:, 0]][:, :, None, None, None], mem[r[:, 1]][:, None, :, None, None],
                                mem[r[:, 2]][:, None, None, :, None], mem[r[:, 3]][:, None, None, None, :])
        lin = np.stack(g, -1).reshape(-1, 4).astype(np.uint32)
        eng.resolve(lin, subsample_snps=False)
        _, a, _, _ = eng.timing_read_split()
        scan_ms += a
    eng.timing_enable(False)
    for f in forms.values():
        f["naive_over_pool"] = round(scan_ms / f["pool_ms"], 2)
    return dict(K=K, lineages=n, T=T, S=S, species_quartets=len(rows), lineage_quartets=total_lin,
                naive_scan_ms=round(scan_ms, 3), **forms)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 5
    with QuartetEngine(0) as eng:
        res = dict(tool="species_bench", reps=reps, shapes=[bench_shape(eng, K, n, reps) for K, n in SHAPES])
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
