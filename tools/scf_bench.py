#!/usr/bin/env python
"""Time the site concordance accumulator on the device (tetrad_amd/scf.py, csrc/scf.hpp).

At the c3 shape (128 taxa x 50 000 SNPs), 1e6 ascending sets, on a random binary tree, medians of `reps` by HIP events
on the call's stream:
  1. `tq_patterns_dev` alone (site scan + class kernel: what produces the rows);
  2. `tq_scf_add_dev` alone on those rows (the scf kernel + the fold kernel);
  3. `tq_conc_add_dev` on as many rows of the same sets: the yardstick of the same structure;
  4. `run_scf` with per_edge=100 at the c3 shape, and with all C(64,4) quartets of a 64-taxon matrix (wall clock).

    python tools/scf_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE).  No threshold is applied to any figure."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import synth  # noqa: E402
from tetrad_amd.concordance import Concordance  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402
from tetrad_amd.scf import SiteConcordance, run_scf  # noqa: E402

T, S, Q = 128, 50_000, 1_000_000


def tree_parent(ntaxa, seed):
    children, _ = synth.random_tree_children(ntaxa, np.random.default_rng(seed))
    parent = np.full(2 * ntaxa - 1, -1, np.int32)
    for v, (a, b) in children.items():
        parent[a] = parent[b] = v
    return parent


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
    return float(np.median(out)), float(np.min(out))


def bench_kernels(eng, reps):
    import torch
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    eng.set_data(tmparr, tmpmap)
    parent = tree_parent(T, 1)
    sets = np.sort(synth.random_quartets(T, Q, seed=7).astype(np.uint32), axis=1)
    d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
    d_classes = torch.empty((Q, 16), dtype=torch.int32, device="cuda")
    cs = torch.cuda.current_stream().cuda_stream
    res = {}
    pat = event_ms(torch, lambda: eng.patterns_dev(d_sets.data_ptr(), Q, False, d_classes.data_ptr(), cs), reps)
    res["patterns_ms"] = dict(median=round(pat[0], 4), min=round(pat[1], 4))
    with SiteConcordance(parent, ntaxa=T, engine=eng) as acc:
        add = event_ms(torch, lambda: acc.add_dev_ptrs(d_sets.data_ptr(), d_classes.data_ptr(), Q, cs), reps)
        st = acc.stats()
        res["scf_add_ms"] = dict(median=round(add[0], 4), min=round(add[1], 4))
        res["scf_add_useful_bytes_per_row"] = 28
        res["scf_add_line_bytes_per_row"] = 80
        res["scf_add_line_GBps"] = round(Q * 80 / add[0] / 1e6, 1) if add[0] > 0 else None
        res["induced_rows_per_add"] = int((st["nq"] + st["nq_zero"]).sum()) // (reps + 1)
    # the yardstick: the concordance accumulator on the same sets, with engine-like scores
    rng = np.random.default_rng(T)
    sc = torch.from_numpy(rng.gamma(4.0, 50.0, size=(Q, 3))).cuda()
    rs = torch.from_numpy(np.stack([rng.integers(0, 3, Q), rng.integers(0, 3000, Q)], axis=1).astype(np.int32)).cuda()
    fl = torch.zeros(Q, dtype=torch.uint8, device="cuda")
    conc = Concordance(parent, ntaxa=T, min_ratio=1.1, engine=eng)
    ca = event_ms(torch, lambda: conc.add_dev_ptrs(d_sets.data_ptr(), rs.data_ptr(), sc.data_ptr(), fl.data_ptr(), Q, cs),
                  reps)
    conc.close()
    res["conc_add_ms"] = dict(median=round(ca[0], 4), min=round(ca[1], 4))
    return res


def bench_run(eng, reps):
    out = {}
    cases = (("per_edge_100_T128", T, S, 100), ("all_quartets_T64", 64, S, None))
    for name, ntaxa, nsites, per_edge in cases:
        tmparr, tmpmap = synth.simulate_tmparr(ntaxa, nsites, seed=103)
        parent = tree_parent(ntaxa, 1)
        walls, rows = [], 0
        for r in range(reps + 1):
            t0 = time.perf_counter()
            stats, _, acc = run_scf(eng, tmparr, tmpmap, parent, per_edge=per_edge, seed=r)
            walls.append(time.perf_counter() - t0)
            rows = int((stats["nq"] + stats["nq_zero"]).sum())
            acc.close()
        out[name] = dict(T=ntaxa, S=nsites, wall_ms=round(float(np.median(walls[1:])) * 1e3, 3), induced_rows=rows,
                         mean_sCF=round(float(np.nanmean(stats["sCF"])), 3))
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
        res = dict(tool="scf_bench", reps=reps, shape=dict(T=T, S=S, sets=Q), kernels=bench_kernels(eng, reps))
    with QuartetEngine(0) as eng:
        res["run_scf"] = bench_run(eng, reps)
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
