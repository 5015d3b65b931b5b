"""Collate two `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE) of `python bench.py --full --no-cpu`
into profiles/traffic_<cfg>_<mode>.json, which bench.py reads for roofline.traffic.

    rocprofv3 --kernel-trace --pmc FETCH_SIZE -d out/pmc_f --output-format csv -- python bench.py --full --no-cpu --steps 4 --warmup 1
    rocprofv3 --kernel-trace --pmc WRITE_SIZE -d out/pmc_w --output-format csv -- python bench.py --full --no-cpu --steps 4 --warmup 1
    python tools/pmc_traffic.py out/pmc_f out/pmc_w --out profiles/traffic_c3_sub.json

Units and corrections follow MI355X_MICROARCH.md (HBM / rocprofv3 section): both counters are in
KiB-like units of 1 KB per count; on gfx950 FETCH_SIZE counts 128-byte requests as 64 bytes, so it
is doubled; WRITE_SIZE is used as reported.  `passes` = resolve passes the profiled command made
(warmup + steps, plus the PCIe-inclusive legs if they ran); the figure is per pass.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from collections import defaultdict
from pathlib import Path

GROUPS = ("tq_prepare", "tq_key", "tq_dp_", "tq_scan_wg", "tq_scan_f4", "tq_scan_dp", "tq_scan_kernel", "tq_bidiag", "tq_bdsqr", "tq_score", "tq_svd",
          "rocprim")


def group_of(name: str) -> str:
    for g in GROUPS:
        if g in name:
            return g
    return "other"


def collect(d: Path, counter: str):
    files = sorted(d.rglob("*counter_collection.csv"))
    if not files:
        sys.exit(f"no *counter_collection.csv under {d}")
    tot, calls = defaultdict(float), defaultdict(int)
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if row["Counter_Name"] != counter:
                    continue
                g = group_of(row["Kernel_Name"])
                tot[g] += float(row["Counter_Value"])
                calls[g] += 1
    return tot, calls, files[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fetch_dir", type=Path)
    ap.add_argument("write_dir", type=Path)
    ap.add_argument("--passes", type=int, default=0,
                    help="resolve passes made by the profiled command (default: dispatches of the scan kernel)")
    ap.add_argument("--config", default="c3 sub, 1e6 quartets per launch")
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--copy-to", type=Path, default=None, help="directory that receives the two csv files")
    ap.add_argument("--commit", default="", help="commit the profiled library was built from")
    args = ap.parse_args()
    ft, fc, ff = collect(args.fetch_dir, "FETCH_SIZE")
    wt, wc, wf = collect(args.write_dir, "WRITE_SIZE")
    if not args.passes:
        scans = ("tq_scan_f4", "tq_scan_wg", "tq_scan_dp", "tq_scan_kernel")
        args.passes = next((fc[g] for g in scans if fc.get(g)), 0)
        if args.passes != next((wc[g] for g in scans if wc.get(g)), 0):
            sys.exit("the two runs made different numbers of passes")
    hot = [g for g in ft if g.startswith("tq_") and g != "tq_prepare"] + ["rocprim"]
    fetch_kb = sum(ft.get(g, 0.0) for g in hot) / args.passes
    write_kb = sum(wt.get(g, 0.0) for g in hot) / args.passes
    out = {
        "config": args.config,
        "commit": args.commit or "unknown",
        "passes": args.passes,
        "fetch_size_kb_per_pass": fetch_kb,
        "write_size_kb_per_pass": write_kb,
        "correction": "FETCH_SIZE x2 (gfx950 counts 128-B requests at 64 B, MI355X_MICROARCH.md HBM section); "
                      "WRITE_SIZE exact; rocprofv3 --pmc in two separate passes; 1 count = 1 KB",
        "hbm_bytes_per_launch": (2.0 * fetch_kb + write_kb) * 1024.0,
        "per_kernel_fetch_kb": {g: ft[g] / args.passes for g in ft},
        "per_kernel_write_kb": {g: wt[g] / args.passes for g in wt},
        "dispatches": {g: fc[g] for g in fc},
    }
    args.out.write_text(json.dumps(out, indent=1) + "\n")
    if args.copy_to:
        args.copy_to.mkdir(parents=True, exist_ok=True)
        (args.copy_to / "pmc_FETCH_SIZE.csv").write_bytes(ff.read_bytes())
        (args.copy_to / "pmc_WRITE_SIZE.csv").write_bytes(wf.read_bytes())
    print(json.dumps({k: out[k] for k in ("fetch_size_kb_per_pass", "write_size_kb_per_pass", "hbm_bytes_per_launch")}))


if __name__ == "__main__":
    main()
