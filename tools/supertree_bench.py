#!/usr/bin/env python
"""Exact supertree on the device, measured.

  stages (default)  rows -> tree for a c5-shape replicate (T = 128, 1e6 rows, strategy 1): the add kernel (HIP events),
                    per level the graph pass, the host search and the partition pass (wall clock of the build thread,
                    synchronisation included: `tq_stree_level_stats`), with the graph pass in its LDS and its
                    global-atomic form; in the same process the host execution of the same rule and the existing host
                    path (`qmc.infer_supertree_from_arrays`, one thread) on the same rows.
  --loop            `bootstrap_trees` at the c5 shape (1e6 quartets per replicate): replicates/s for supertree="host"
                    and "device" in alternating rounds, workers 2 and 8, and the replicate loop without trees.

  --search          the cut search rules on device rows, in alternating rounds in one run: the f64
                    rule with its host search, the exact rule on the host (option stree_search_dev = 0) and the exact
                    rule in the search kernel; rows -> tree and per level graph / search / partition ms at the c5
                    shape (T = 128) and at T = 512.  With --loop: replicates/s of `bootstrap_trees(supertree="device")`
                    for the same three legs.

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


def stages(args):
    import torch
    from supertree_model import bipartitions, newick_bipartitions, rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    T, n = 128, args.rows
    children, root, q, sc, st = rows_from_tree(T, n, "random", 0.1, seed=5)
    truth = bipartitions(children, root, T)
    out = {"T": T, "rows": n, "weights": 1, "reps": args.reps}
    with QuartetEngine(0) as eng:
        dq = torch.from_numpy(q.view(np.int32)).cuda()
        dst = torch.from_numpy(st.view(np.int32)).cuda()
        dsc = torch.from_numpy(sc).cuda()
        cur = torch.cuda.current_stream()
        with qmc.Supertree(T, n, 1, engine=eng) as acc:
            add_ms = []
            for _ in range(args.reps + 1):
                acc.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                acc.add_dev_ptrs(dq.data_ptr(), dst.data_ptr(), dsc.data_ptr(), 0, n, cur.cuda_stream)
                e1.record(cur)
                e1.synchronize()
                add_ms.append(e0.elapsed_time(e1))
            out["add_kernel_ms"] = med(add_ms[1:])
            for lds in (1, 0):
                eng.set_option("stree_lds", lds)
                total, levels = [], []
                for r in range(args.reps + 1):
                    t0 = time.perf_counter()
                    nwk = acc.tree(seed=r, stream=cur.cuda_stream)
                    total.append((time.perf_counter() - t0) * 1e3)
                    levels.append(acc.level_stats())
                L = min(len(x) for x in levels[1:])
                per = np.median(np.stack([x[:L] for x in levels[1:]]), axis=0)
                out["device_lds" if lds else "device_global"] = {
                    "tree_ms": med(total[1:]), "tree_ms_min_max": [round(min(total[1:]), 3), round(max(total[1:]), 3)],
                    "graph_ms": round(float(per[:, 3].sum()), 3), "search_ms": round(float(per[:, 4].sum()), 3),
                    "partition_ms": round(float(per[:, 5].sum()), 3),
                    "levels": [dict(level=i, nodes=int(p[0]), live=int(p[1]), cells=int(p[2]), graph_ms=round(p[3], 4),
                                    search_ms=round(p[4], 4), partition_ms=round(p[5], 4)) for i, p in enumerate(per)],
                    "true_bipartitions": [len(newick_bipartitions(nwk, T) & truth), len(truth)]}
            eng.set_option("stree_lds", 1)
            dev_nwk = acc.tree(seed=3, stream=cur.cuda_stream)
    with qmc.Supertree(T, n, 1) as host:
        t0 = time.perf_counter()
        host.add(q, sc, st)
        out["host_exact_add_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        ts = []
        for r in range(3):
            t0 = time.perf_counter()
            nwk = host.tree(seed=3)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["host_exact_tree_ms"] = med(ts)
        out["device_equals_host_string"] = bool(nwk == dev_nwk)
    ts = []
    for r in range(3):
        t0 = time.perf_counter()
        nwk = qmc.infer_supertree_from_arrays(q, sc, st, T, 1, seed=r)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["host_path_tq_qmc_tree_ms"] = med(ts)
    out["host_path_true_bipartitions"] = [len(newick_bipartitions(nwk, T) & truth), len(truth)]
    return out


def loop(args):
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd.replicates import ReplicateRunner, bootstrap_trees
    seqarr, maparr, spans = synth.make_c5_source()
    Q, nb = 1_000_000, args.nboots
    out = {"quartets": Q, "replicates": nb, "rounds": args.rounds, "sampler": args.sampler}
    with QuartetEngine(0) as eng:
        bootstrap_trees(eng, seqarr, spans, Q, 3, weights=1, seed=1, sampler=args.sampler, workers=2, supertree="device")
        bootstrap_trees(eng, seqarr, spans, Q, 3, weights=1, seed=1, sampler=args.sampler, workers=2, supertree="host")
        for workers in (2, 8):
            rates = {"host": [], "device": []}
            for r in range(args.rounds):
                for mode in ("host", "device"):
                    t0 = time.perf_counter()
                    trees = bootstrap_trees(eng, seqarr, spans, Q, nb, weights=1, seed=2 + r, sampler=args.sampler,
                                            workers=workers, supertree=mode)
                    rates[mode].append(len(trees) / (time.perf_counter() - t0))
            out[f"workers_{workers}"] = {m: {"replicates_per_s": med(v), "rounds": [round(x, 2) for x in v]}
                                         for m, v in rates.items()}
        rates = []
        for r in range(args.rounds):
            runner = ReplicateRunner(eng, seqarr, spans, Q, seed=2 + r, sampler=args.sampler)
            t0 = time.perf_counter()
            runner.run(nb, True)
            rates.append(nb / (time.perf_counter() - t0))
            runner.close()
        out["loop_without_trees"] = {"replicates_per_s": med(rates), "rounds": [round(x, 2) for x in rates]}
    return out


SEARCH_LEGS = (("f64", "f64", 1), ("exact_host", "exact", 0), ("exact_device", "exact", 1))


def search_stages(args):
    import torch
    from supertree_model import bipartitions, newick_bipartitions, rows_from_tree
    from tetrad_amd import qmc
    from tetrad_amd.engine import QuartetEngine
    out = {"reps": args.reps, "rows": args.rows, "weights": 1}
    with QuartetEngine(0) as eng:
        cur = torch.cuda.current_stream()
        for T in (128, 512):
            children, root, q, sc, st = rows_from_tree(T, args.rows, "random", 0.1, seed=5)
            truth = bipartitions(children, root, T)
            n = len(q)
            dq = torch.from_numpy(q.view(np.int32)).cuda()
            dst = torch.from_numpy(st.view(np.int32)).cuda()
            dsc = torch.from_numpy(sc).cuda()
            total = {leg: [] for leg, _, _ in SEARCH_LEGS}
            levels = {leg: [] for leg, _, _ in SEARCH_LEGS}
            found = {}
            with qmc.Supertree(T, n, 1, engine=eng) as acc:
                acc.add_dev_ptrs(dq.data_ptr(), dst.data_ptr(), dsc.data_ptr(), 0, n, cur.cuda_stream)
                try:
                    for r in range(args.reps + 1):                             # round 0 warms up
                        for leg, rule, on_dev in SEARCH_LEGS:
                            acc.set_search(rule)
                            eng.set_option("stree_search_dev", on_dev)
                            t0 = time.perf_counter()
                            nwk = acc.tree(seed=r, stream=cur.cuda_stream)
                            if r:
                                total[leg].append((time.perf_counter() - t0) * 1e3)
                                levels[leg].append(acc.level_stats())
                            found[leg] = [len(newick_bipartitions(nwk, T) & truth), len(truth)]
                finally:
                    eng.set_option("stree_search_dev", 1)
            res = {}
            for leg, _, _ in SEARCH_LEGS:
                L = min(len(x) for x in levels[leg])
                per = np.median(np.stack([x[:L] for x in levels[leg]]), axis=0)
                res[leg] = {
                    "tree_ms": med(total[leg]), "tree_ms_min_max": [round(min(total[leg]), 3), round(max(total[leg]), 3)],
                    "graph_ms": round(float(per[:, 3].sum()), 3), "search_ms": round(float(per[:, 4].sum()), 3),
                    "partition_ms": round(float(per[:, 5].sum()), 3), "true_bipartitions": found[leg],
                    "levels": [dict(level=i, nodes=int(p[0]), live=int(p[1]), cells=int(p[2]), graph_ms=round(p[3], 4),
                                    search_ms=round(p[4], 4), partition_ms=round(p[5], 4)) for i, p in enumerate(per)]}
            out[f"T{T}"] = res
    return out


def search_loop(args):
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd.replicates import bootstrap_trees
    seqarr, maparr, spans = synth.make_c5_source()
    Q, nb = 1_000_000, args.nboots
    out = {"quartets": Q, "replicates": nb, "rounds": args.rounds, "sampler": args.sampler, "workers": 8}
    with QuartetEngine(0) as eng:
        rates = {leg: [] for leg, _, _ in SEARCH_LEGS}
        try:
            for r in range(args.rounds + 1):                                   # round 0 warms up
                for leg, rule, on_dev in SEARCH_LEGS:
                    eng.set_option("stree_search_dev", on_dev)
                    t0 = time.perf_counter()
                    trees = bootstrap_trees(eng, seqarr, spans, Q, nb if r else 3, weights=1, seed=2 + r,
                                            sampler=args.sampler, workers=8, supertree="device", search=rule)
                    if r:
                        rates[leg].append(len(trees) / (time.perf_counter() - t0))
        finally:
            eng.set_option("stree_search_dev", 1)
        for leg, v in rates.items():
            out[leg] = {"replicates_per_s": med(v), "rounds": [round(x, 2) for x in v]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nboots", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sampler", default="device")
    ap.add_argument("--out")
    args = ap.parse_args()
    from tetrad_amd import _lib
    res = {"commit": (REPO / ".build_commit").read_text().strip() if (REPO / ".build_commit").exists() else None,
           "library": str(_lib.LIB_PATH.name)}
    if args.search:
        res["search_loop" if args.loop else "search_stages"] = search_loop(args) if args.loop else search_stages(args)
    else:
        res["loop" if args.loop else "stages"] = loop(args) if args.loop else stages(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
