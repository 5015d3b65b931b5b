#!/usr/bin/env python
"""Quartet fit and best-of-N supertree builds, measured.

  stages (default)  c5 shape (T = 128, 1e6 rows, strategy 1, 10 % wrong rows), medians of --reps:
                    * `tq_stree_fit` of R = 1, 8 and 32 trees on device rows, by HIP events on the call's stream (the
                      whole span: upload of the parent arrays, table kernel, fit kernel, download) and by wall clock;
                      the same call on an accumulator whose device rows are all skipped (kept = 0: every workgroup of
                      the fit kernel returns at once), which leaves the upload and `tq_fit_table_kernel`; the
                      difference of the two is `tq_fit_kernel`;
                    * the host execution of the same fits on the same rows;
                    * `tree(restarts=8)` against `tree()` in alternating rounds.
  --loop            `bootstrap_trees(supertree="device")` at the c5 shape with restarts 1, 4 and 8 in alternating
                    rounds: replicates/s.
  --quality         one noisy input (T = 128, 40 % wrong rows): the satisfied fraction of the trees of 8 seeds for
                    search="f64" and for search="exact", and of the best of the 8.

Run each mode as a step of its own under a time limit, e.g. `timeout -k 10 300 python tools/fit_bench.py --out ...`.
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


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return {"median": med(xs), "min_max": [round(min(xs), 4), round(max(xs), 4)]}


def dev_rows(q, sc, st, fl=None):
    import torch
    return (torch.from_numpy(q.view(np.int32)).cuda(), torch.from_numpy(st.view(np.int32)).cuda(),
            torch.from_numpy(sc).cuda(), None if fl is None else torch.from_numpy(fl).cuda())


def add(acc, d, stream):
    dq, dst, dsc, dfl = d
    acc.add_dev_ptrs(dq.data_ptr(), dst.data_ptr(), dsc.data_ptr(), 0 if dfl is None else dfl.data_ptr(), dq.shape[0],
                     stream.cuda_stream)


def candidate_trees(T, children, root, R):
    import fit_model as fm
    from supertree_model import tree_children
    gen = fm.parent_from_children(children, root, T)
    trees = [gen]
    for i in range(1, R):
        other = fm.parent_from_children(*tree_children(T, "random", np.random.default_rng(100 + i)), T)
        trees.append(fm.contract(other, T, np.random.default_rng(i), 0.2) if i % 4 == 3 else other)
    return trees


def stages(args):
    import torch
    from supertree_model import bad_rows, rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    T, n = 128, args.rows
    children, root, q, sc, st = rows_from_tree(T, n, "random", 0.1, seed=5)
    trees = candidate_trees(T, children, root, 32)
    out = {"T": T, "rows": n, "weights": 1, "wrong": 0.1, "reps": args.reps}
    with QuartetEngine(0) as eng:
        cur = torch.cuda.current_stream()
        bq, bsc, bst, bfl = bad_rows(T, 7000, np.random.default_rng(1))
        with qmc.Supertree(T, n, 1, engine=eng) as acc, qmc.Supertree(T, 7000, 1, engine=eng) as empty:
            add(acc, dev_rows(q, sc, st), cur)
            add(empty, dev_rows(bq, bsc, bst, bfl), cur)
            assert empty.counts()[0] == 0 and acc.counts()[0] == n
            for R in (1, 8, 32):
                legs = {"fit": acc, "tables_only": empty}
                ev_ms = {k: [] for k in legs}
                wall_ms = {k: [] for k in legs}
                for r in range(args.reps + 1):                              # round 0 warms up (and allocates)
                    for leg, a in legs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0 = time.perf_counter()
                        e0.record(cur)
                        res = a.fit(trees[:R], stream=cur.cuda_stream)
                        e1.record(cur)
                        e1.synchronize()
                        if r:
                            wall_ms[leg].append((time.perf_counter() - t0) * 1e3)
                            ev_ms[leg].append(e0.elapsed_time(e1))
                        if leg == "fit":
                            first = res
                out[f"R{R}"] = {
                    "call_event_ms": spread(ev_ms["fit"]), "call_wall_ms": spread(wall_ms["fit"]),
                    "upload_and_table_kernel_event_ms": spread(ev_ms["tables_only"]),
                    "fit_kernel_ms_by_difference": round(med(ev_ms["fit"]) - med(ev_ms["tables_only"]), 4),
                    "generating_tree_fraction": round(float(first[0]["fraction"]), 6)}
            single, eight = [], []
            for r in range(args.reps + 1):
                t0 = time.perf_counter()
                acc.tree(seed=10 * r, stream=cur.cuda_stream)
                t1 = time.perf_counter()
                acc.tree(seed=10 * r, stream=cur.cuda_stream, restarts=8)
                t2 = time.perf_counter()
                if r:
                    single.append((t1 - t0) * 1e3)
                    eight.append((t2 - t1) * 1e3)
            out["tree_ms"] = spread(single)
            out["tree_restarts8_ms"] = spread(eight)
            dev8 = acc.fit(trees[:8], stream=cur.cuda_stream)
    with qmc.Supertree(T, n, 1) as host:
        host.add(q, sc, st)
        for R in (1, 8, 32):
            ts = []
            for r in range(3):
                t0 = time.perf_counter()
                res = host.fit(trees[:R])
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"R{R}"]["host_execution_ms"] = spread(ts)
            if R == 8:
                out["device_equals_host"] = bool(all((res[f] == dev8[f]).all() for f in res.dtype.names[:6]))
    return out


def loop(args):
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd.replicates import bootstrap_trees
    seqarr, maparr, spans = synth.make_c5_source()
    Q, nb = 1_000_000, args.nboots
    out = {"quartets": Q, "replicates": nb, "rounds": args.rounds, "sampler": args.sampler, "workers": args.workers}
    with QuartetEngine(0) as eng:
        rates = {1: [], 4: [], 8: []}
        gain = {4: [], 8: []}
        for r in range(args.rounds + 1):                                   # round 0 warms up
            fr = {}
            for restarts in rates:
                fits = []
                t0 = time.perf_counter()
                trees = bootstrap_trees(eng, seqarr, spans, Q, nb if r else 3, weights=1, seed=2 + r, sampler=args.sampler,
                                        workers=args.workers, supertree="device", restarts=restarts, fit_out=fits)
                if r:
                    rates[restarts].append(len(trees) / (time.perf_counter() - t0))
                    fr[restarts] = float(np.mean([f["fraction"] for f in fits]))
            for k in gain:
                if r:
                    gain[k].append(fr[k] - fr[1])
        for k, v in rates.items():
            out[f"restarts_{k}"] = {"replicates_per_s": med(v), "rounds": [round(x, 2) for x in v]}
        for k, v in gain.items():
            out[f"restarts_{k}"]["mean_fraction_gain_over_1"] = [round(x, 6) for x in v]
    return out


def quality(args):
    import torch
    from supertree_model import bipartitions, newick_bipartitions, rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    T, n, wrong = 128, args.rows, 0.4
    children, root, q, sc, st = rows_from_tree(T, n, "random", wrong, seed=6)
    truth = bipartitions(children, root, T)
    out = {"T": T, "rows": n, "weights": 1, "wrong": wrong, "seeds": 8}
    with QuartetEngine(0) as eng:
        cur = torch.cuda.current_stream()
        d = dev_rows(q, sc, st)
        for search in ("f64", "exact"):
            with qmc.Supertree(T, n, 1, engine=eng, search=search) as acc:
                add(acc, d, cur)
                best = acc.tree(seed=0, stream=cur.cuda_stream, restarts=8)
                fr = [float(x) for x in acc.last_fit.results["fraction"]]
                out[search] = {"fraction_by_seed": [round(x, 6) for x in fr], "median": round(statistics.median(fr), 6),
                               "min": round(min(fr), 6), "max": round(max(fr), 6), "chosen_seed": acc.last_fit.chosen,
                               "distinct_trees": len({tuple(int(x) for x in r.tolist()[:6]) for r in acc.last_fit.results}),
                               "best_true_bipartitions": [len(newick_bipartitions(best, T) & truth), len(truth)]}
        import fit_model as fm
        with qmc.Supertree(T, n, 1, engine=eng) as acc:
            add(acc, d, cur)
            out["generating_tree_fraction"] = round(float(acc.fit(fm.parent_from_children(children, root, T))["fraction"]), 6)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nboots", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--sampler", default="device")
    ap.add_argument("--out")
    args = ap.parse_args()
    from tetrad_amd import _lib
    res = {"commit": (REPO / ".build_commit").read_text().strip() if (REPO / ".build_commit").exists() else None,
           "library": str(_lib.LIB_PATH.name)}
    if args.loop:
        res["loop"] = loop(args)
    elif args.quality:
        res["quality"] = quality(args)
    else:
        res["stages"] = stages(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
