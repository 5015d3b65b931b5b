#!/usr/bin/env python
"""Time the concordance accumulator on the device (tetrad_amd/concordance.py, csrc/concordance.hpp).

  1. `Concordance.add_dev` on 1e6 c3-shaped rows (random quartets of T taxa, engine-like scores), HIP events around
     each add (the conc kernel + the fold kernel), at T = 128 (LDS table) and T = 600 (table through L2);
  2. the c5 replicate loop (bootstrap replicate built on the device, 1e6-quartet sample, resolve) with and without
     `concordance=`: wall time per replicate, alternating the two legs so that drift hits both.

    python tools/concordance_bench.py [reps] [replicates]
Prints one JSON line."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tetrad_amd import synth  # noqa: E402
from tetrad_amd.concordance import Concordance  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402
from tetrad_amd.replicates import ReplicateRunner  # noqa: E402


def tree_parent(T, seed):
    children, root = synth.random_tree_children(T, np.random.default_rng(seed))
    parent = np.full(2 * T - 1, -1, np.int32)
    for v, (a, b) in children.items():
        parent[a] = parent[b] = v
    return parent


def time_add(eng, T, n, reps):
    rng = np.random.default_rng(T)
    q = np.stack([rng.permutation(T)[:4] for _ in range(4096)])[rng.integers(0, 4096, n)].astype(np.int32)
    sc = rng.gamma(4.0, 50.0, size=(n, 3))
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 3000, n)], axis=1).astype(np.int32)
    d = [torch.from_numpy(a).cuda() for a in (q, st, sc, np.zeros(n, np.uint8))]
    acc = Concordance(tree_parent(T, 1), ntaxa=T, min_ratio=1.1, engine=eng)
    for _ in range(3):
        acc.add_dev(*d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        acc.add_dev(*d)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    acc.close()
    return dict(T=T, rows=n, bytes_per_row=49, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)),
                rows_per_s=n / (np.median(ms) * 1e-3))


def time_loop(eng, nrep, rounds):
    seqarr, _, spans = synth.make_c5_source()
    T = seqarr.shape[0]
    acc = Concordance(tree_parent(T, synth.CONFIG_SEEDS["c5"]), ntaxa=T, min_ratio=1.1, engine=eng)
    out = {"off": [], "on": []}
    for r in range(rounds):
        for leg in ("off", "on"):
            runner = ReplicateRunner(eng, seqarr, spans, 1_000_000, seed=synth.CONFIG_SEEDS["c5"] + r,
                                     concordance=acc if leg == "on" else None)
            runner.run(1, True)                                   # warm-up replicate
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.run(nrep, True)
            torch.cuda.synchronize()
            out[leg].append((time.perf_counter() - t0) * 1e3 / nrep)
            runner.close()
    s = acc.stats()
    return dict(T=T, quartets=1_000_000, replicates_per_leg=nrep, rounds=rounds,
                ms_per_replicate_off=out["off"], ms_per_replicate_on=out["on"],
                median_off=float(np.median(out["off"])), median_on=float(np.median(out["on"])),
                induced_rows=int((s["conc"] + s["disc1"] + s["disc2"] + s["nu"]).sum()))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    nrep = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    with QuartetEngine(0) as eng:
        res = dict(add=[time_add(eng, 128, 1_000_000, reps), time_add(eng, 600, 1_000_000, reps)],
                   loop=time_loop(eng, nrep, 3), device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
