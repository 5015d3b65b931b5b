#!/usr/bin/env python
"""Time the five-taxon block rows (tetrad_amd/quintets.py, csrc/quintet_blocks.hpp) against the four-taxon ones.

At the c3 shape (128 taxa x 50 000 SNPs), full mode, medians of `reps` by HIP events on the call's stream, all in one
process, at B = 1, 20 and 50 equal blocks:
  1. `tq_patterns_quintet_blocks_dev` on 1e6 ascending five-sets;
  2. `tq_patterns_blocks_dev` on 1e6 ascending four-sets: the kernel of the parent commit, the yardstick (the new one
     issues 5 loads per word against 4 and 10 difference words against 6).
The two are timed in turns (one repetition of each, `reps` times) after a warm-up of both, rows in chunks of sets that
keep the output below 1 GiB, the chunks' times summed.  Then `tq_dstat_jackknife_masks_dev` at B = 50 on four tests per
set (the four DFOIL statistics of the ascending roles) of the chunk the last call left, against `tq_dstat_jackknife_dev`
on the same number of tests of the four-taxon rows.

    python tools/quintet_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import quintets, synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

T, S, Q = 128, 50_000, 1_000_000
OUT_BYTES = 1 << 30


def random_sets(width, seed):
    """Q strictly ascending rows of `width` distinct taxa, uniform over the taxa."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, T, size=(Q, width))
    while True:
        rows.sort(axis=1)
        dup = (rows[:, 1:] == rows[:, :-1]).any(axis=1)
        if not dup.any():
            return np.ascontiguousarray(rows, dtype=np.uint32)
        rows[dup] = rng.integers(0, T, size=(int(dup.sum()), width))


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def in_turns(torch, fns, reps):
    """Median ms of each callable: a warm-up of all, then `reps` rounds of one timed repetition of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(timed(torch, fn))
    return [float(np.median(m)) for m in ms]


def bench(eng, reps):
    import torch
    tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=103)
    eng.set_data(tmparr, tmpmap)
    sets4, sets5 = random_sets(4, 7), random_sets(5, 8)
    d4 = torch.from_numpy(sets4.view(np.int32)).cuda()
    d5 = torch.from_numpy(sets5.view(np.int32)).cuda()
    cs = torch.cuda.current_stream().cuda_stream
    res = {}
    for B in (1, 20, 50):
        starts = np.linspace(0, S, B + 1).astype(np.int64)
        chunk = min(Q, OUT_BYTES // (B * 64))
        d_rows4 = torch.empty((chunk, B, 16), dtype=torch.int32, device="cuda")
        d_rows5 = torch.empty((chunk, B, 16), dtype=torch.int32, device="cuda")

        def rows4():
            for q0 in range(0, Q, chunk):
                eng.patterns_blocks_dev(d4.data_ptr() + 16 * q0, min(chunk, Q - q0), starts, d_rows4.data_ptr(), cs)

        def rows5():
            for q0 in range(0, Q, chunk):
                eng.patterns_quintet_blocks_dev(d5.data_ptr() + 20 * q0, min(chunk, Q - q0), starts, d_rows5.data_ptr(), cs)

        m5, m4 = in_turns(torch, [rows5, rows4], reps)
        res[f"quintet_blocks_B{B}_ms"] = round(m5, 4)
        res[f"quartet_blocks_B{B}_ms"] = round(m4, 4)
        res[f"ratio_B{B}"] = round(m5 / m4, 4)
        if B == 1:                                                  # slot 0 is the sum of the 15 classes
            assert torch.equal(d_rows5[:, 0, 0], d_rows5[:, 0, 1:].sum(dim=1, dtype=torch.int32))
            res["quintet_counted_sites_per_set"] = round(d_rows5[:, 0, 0].sum(dtype=torch.int64).item() / Q, 2)
        if B == 50:
            n_sets = min(chunk, Q - (Q - 1) // chunk * chunk)       # the chunk the last calls left in the rows
            N = 4 * n_sets
            _, _, masks = quintets.quintet_tests(np.array([[0, 1, 2, 3, 4]]), quintets.DFOIL)
            d_set_of = torch.from_numpy(np.repeat(np.arange(n_sets, dtype=np.int32), 4)).cuda()
            d_l = torch.from_numpy(np.tile(masks[0, :, 0], n_sets).view(np.int16)).cuda()
            d_r = torch.from_numpy(np.tile(masks[0, :, 1], n_sets).view(np.int16)).cuda()
            d_ia = torch.from_numpy(np.tile(np.array([8, 6, 3, 8], np.uint8), n_sets)).cuda()
            d_ib = torch.from_numpy(np.tile(np.array([6, 3, 8, 3], np.uint8), n_sets)).cuda()
            d_out = torch.empty((N, 4), dtype=torch.float64, device="cuda")
            mm, mc = in_turns(torch, [
                lambda: eng.dstat_jackknife_masks_dev(d_rows5.data_ptr(), n_sets, B, d_set_of.data_ptr(), d_l.data_ptr(),
                                                      d_r.data_ptr(), N, d_out.data_ptr(), cs),
                lambda: eng.dstat_jackknife_dev(d_rows4.data_ptr(), n_sets, B, d_set_of.data_ptr(), d_ia.data_ptr(),
                                                d_ib.data_ptr(), N, d_out.data_ptr(), cs)], reps)
            res["jackknife_B50_tests"] = N
            res["jackknife_masks_B50_ms"] = round(mm, 4)
            res["jackknife_classes_B50_ms"] = round(mc, 4)
        del d_rows4, d_rows5
    return res


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 7
    with QuartetEngine(0) as eng:
        res = dict(tool="quintet_bench", reps=reps, shape=dict(T=T, S=S, sets=Q), kernels=bench(eng, reps))
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
