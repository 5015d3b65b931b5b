#!/usr/bin/env python
"""NNI scan and polish of supertrees, measured at the c5 shape: T = 128, 1e6 rows, strategy 1,
with 10 % and with 40 % wrong rows, everything in one process per mode.

  scan (default)  per input, on the tree that `tree(seed=0)` builds:
                  (a) one `nni_scan` on device rows by HIP events on the call's stream (the whole span: upload of the
                      parent and edge records, table kernel, scan kernel, download) and by wall clock: the median of
                      --reps after a warm-up;
                  (b) `tq_stree_fit` of the 2 (T - 3) neighbour trees of the same tree, which is how the same numbers
                      are obtained without the scan, timed the same way (median of 3); the tool asserts that every
                      neighbour's fit equals the tree's fit shifted by the scanned weights.
  --search        (c) per input and search rule: `polish` on the builds of 8 seeds -- wall clock, rounds, interchanges,
                  satisfied fraction before and after -- next to `tree(restarts=8)` without polish and with it.

Run each mode as a step of its own under a time limit, e.g. `timeout -k 10 300 python tools/polish_bench.py --out ...`.
Prints one JSON document; --out FILE also writes it."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

WRONG = (0.1, 0.4)


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return {"median": med(xs), "min_max": [round(min(xs), 4), round(max(xs), 4)]}


def dev_rows(q, sc, st):
    import torch
    return (torch.from_numpy(q.view(np.int32)).cuda(), torch.from_numpy(st.view(np.int32)).cuda(),
            torch.from_numpy(sc).cuda())


def add(acc, d, stream):
    dq, dst, dsc = d
    acc.add_dev_ptrs(dq.data_ptr(), dst.data_ptr(), dsc.data_ptr(), 0, dq.shape[0], stream.cuda_stream)


def timed(cur, reps, call):
    """(event ms, wall ms, last result) of `reps` calls after one warm-up"""
    import torch
    ev, wall, res = [], [], None
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(cur)
        res = call()
        e1.record(cur)
        e1.synchronize()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
    return ev, wall, res


def scan(args):
    import torch
    import nni_model as nm
    from supertree_model import rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    T, n = 128, args.rows
    out = {"T": T, "rows": n, "weights": 1, "reps": args.reps}
    with QuartetEngine(0) as eng:
        cur = torch.cuda.current_stream()
        for wrong in WRONG:
            q, sc, st = rows_from_tree(T, n, "random", wrong, seed=5)[2:]
            with qmc.Supertree(T, n, 1, engine=eng) as acc:
                add(acc, dev_rows(q, sc, st), cur)
                nwk = acc.tree(seed=0, stream=cur.cuda_stream)
                ev, wall, rec = timed(cur, args.reps, lambda: acc.nni_scan(nwk, stream=cur.cuda_stream))
                par = acc._parent_of(nwk, None)
                neigh = nm.all_neighbours(par, T)
                trees = [p for _, _, p in neigh]
                fev, fwall, fits = timed(cur, 3, lambda: acc.fit(trees, stream=cur.cuda_stream))
                base = acc.fit(nwk, stream=cur.cuda_stream)
                for (e, alt, _), f in zip(neigh, fits):
                    w0, wa = int(rec[e]["w0"]), int(rec[e][f"w{alt}"])
                    assert int(f["k_satisfied"]) == int(base["k_satisfied"]) - w0 + wa, (e, alt)
                    assert int(f["k_violated"]) == int(base["k_violated"]) + w0 - wa, (e, alt)
                    assert int(f["k_unresolved"]) == int(base["k_unresolved"])
                cand = sum(1 for r in rec if max(int(r["w1"]), int(r["w2"])) > int(r["w0"]))
                out[f"wrong_{wrong}"] = {
                    "edges": len(rec), "eligible": int(rec["eligible"].sum()), "candidates": cand,
                    "scan_event_ms": spread(ev), "scan_wall_ms": spread(wall),
                    "neighbours": len(trees), "fit_of_neighbours_event_ms": spread(fev),
                    "fit_of_neighbours_wall_ms": spread(fwall), "scan_equals_fit_of_neighbours": True,
                    "speedup_by_event_medians": round(med(fev) / med(ev), 1)}
    return out


def search(args):
    import torch
    from supertree_model import rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    T, n, seeds = 128, args.rows, 8
    out = {"T": T, "rows": n, "weights": 1, "seeds": seeds}
    with QuartetEngine(0) as eng:
        cur = torch.cuda.current_stream()
        for wrong in WRONG:
            q, sc, st = rows_from_tree(T, n, "random", wrong, seed=5)[2:]
            d = dev_rows(q, sc, st)
            for rule in ("f64", "exact"):
                with qmc.Supertree(T, n, 1, engine=eng, search=rule) as acc:
                    add(acc, d, cur)
                    acc.polish(acc.tree(seed=99, stream=cur.cuda_stream), stream=cur.cuda_stream)      # warm-up, allocates
                    ms, rounds, moves, before, after, build_ms = [], [], [], [], [], []
                    for s in range(seeds):
                        t0 = time.perf_counter()
                        nwk = acc.tree(seed=s, stream=cur.cuda_stream)
                        t1 = time.perf_counter()
                        pol, trace = acc.polish(nwk, stream=cur.cuda_stream)
                        t2 = time.perf_counter()
                        build_ms.append((t1 - t0) * 1e3)
                        ms.append((t2 - t1) * 1e3)
                        rounds.append(len(trace.moves))
                        moves.append(sum(trace.moves))
                        fb, fa = acc.fit([nwk, pol], stream=cur.cuda_stream)
                        assert trace.converged and int(fa["k_satisfied"]) - int(fb["k_satisfied"]) == sum(trace.gains)
                        before.append(float(fb["fraction"]))
                        after.append(float(fa["fraction"]))
                    t0 = time.perf_counter()
                    acc.tree(seed=0, stream=cur.cuda_stream, restarts=seeds)
                    t1 = time.perf_counter()
                    best_plain = float(acc.last_fit.results[acc.last_fit.chosen]["fraction"])
                    acc.tree(seed=0, stream=cur.cuda_stream, restarts=seeds, polish=True)
                    t2 = time.perf_counter()
                    best_pol = float(acc.last_fit.results[acc.last_fit.chosen]["fraction"])
                    out[f"wrong_{wrong}_{rule}"] = {
                        "build_wall_ms": spread(build_ms), "polish_wall_ms": spread(ms), "rounds": rounds, "moves": moves,
                        "fraction_before": [round(x, 6) for x in before], "fraction_after": [round(x, 6) for x in after],
                        "median_fraction_before": round(statistics.median(before), 6),
                        "median_fraction_after": round(statistics.median(after), 6),
                        "restarts8_wall_ms": round((t1 - t0) * 1e3, 2), "restarts8_fraction": round(best_plain, 6),
                        "restarts8_polish_wall_ms": round((t2 - t1) * 1e3, 2), "restarts8_polish_fraction": round(best_pol, 6)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    from tetrad_amd import _lib
    res = {"library": str(_lib.LIB_PATH.name)}
    if args.search:
        res["search"] = search(args)
    else:
        res["scan"] = scan(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
