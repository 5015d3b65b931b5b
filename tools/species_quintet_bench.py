#!/usr/bin/env python
"""Time the pooled five-taxon block rows of species sets (tetrad_amd/csrc/species_quintet_blocks.hpp).

Two shapes, both 128 samples x 50 000 sites: K = 16 species x 8 lineages with all C(16,5) = 4 368 species sets, and K = 32 x 4
with all C(32,5) = 201 376 (the tool takes at most 1e6 sets of a shape).  At B = 1, 20 and 50 equal blocks three calls are
timed in the same process and in turns (one timing of each per round, `reps` rounds, medians), by HIP events on the call's
stream:
  1. `tq_patterns_quintet_blocks_species_dev` on all the sets (rows in chunks of sets that keep the output below 1 GiB, the
     chunks' times summed);
  2. `tq_patterns_blocks_species_dev`, the four-species sibling, on as many four-sets (the first four ids of every set);
  3. the other way to get such rows: the n^5 lineage quintets of a 1 000-set sample through `tq_patterns_quintet_blocks_dev`
     at the same B, in chunks below 1 GiB of rows, SCALED up to all sets (the sum over the quintets not included).
Before the timing the tool checks, at B = 1, that the rows of the first sampled set equal the sum of its lineage quintets'
rows.

    python tools/species_quintet_bench.py [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
from itertools import combinations, islice
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

S = 50_000
SHAPES = ((16, 8), (32, 4))
MAX_SETS = 1_000_000
OUT_BYTES = 1 << 30
SAMPLE = 1000
BLOCKS = (1, 20, 50)


def shape_inputs(K, n_per):
    """(tmparr, tmpmap, species_of, ssets5 u32[Q,5], picked set indices, their lineage quintets u32[P * n^5, 5])"""
    tmparr, tmpmap, sp, _ = synth.simulate_species(K, n_per, S, seed=100 + K)
    ssets = np.array(list(islice(combinations(range(K), 5), MAX_SETS)), np.uint32)
    rng = np.random.default_rng(K)
    pick = np.sort(rng.choice(len(ssets), size=min(SAMPLE, len(ssets)), replace=False))
    mem = [np.flatnonzero(sp == k).astype(np.uint32) for k in range(K)]
    lin = np.empty((len(pick), n_per ** 5, 5), np.uint32)
    for i, s in enumerate(ssets[pick]):
        lin[i] = np.stack(np.meshgrid(*(mem[int(k)] for k in s), indexing="ij"), axis=-1).reshape(-1, 5)
    return tmparr, tmpmap, sp, ssets, pick, lin.reshape(-1, 5)


def timed_in_turns(torch, fns, reps):
    """Medians of `reps` event timings of every call in `fns` (name -> callable), one of each per round."""
    for fn in fns.values():                                         # warm-up: allocations, first launch, the species table
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return {name: float(np.median(v)) for name, v in out.items()}


def bench_shape(eng, K, n_per, reps, inputs):
    import torch
    tmparr, tmpmap, sp, ssets, pick, lin = inputs
    eng.set_data(tmparr, tmpmap)
    eng.set_species(sp, K)
    Q, P = len(ssets), len(lin)
    per_set = n_per ** 5
    d_sets = torch.from_numpy(ssets.view(np.int32)).cuda()
    d_sets4 = torch.from_numpy(np.ascontiguousarray(ssets[:, :4]).view(np.int32)).cuda()
    d_lin = torch.from_numpy(lin.view(np.int32)).cuda()
    cs = torch.cuda.current_stream().cuda_stream
    res = dict(K=K, lineages=n_per, sets=Q, expansion_sample_sets=len(pick), expansion_quintets=P)
    # the same rows both ways for the first sampled set
    whole = np.array([0, S], np.int64)
    d_one = torch.empty((1, 1, 16), dtype=torch.int32, device="cuda")
    d_exp = torch.empty((per_set, 1, 16), dtype=torch.int32, device="cuda")
    eng.patterns_quintet_blocks_species_dev(d_sets.data_ptr() + 20 * int(pick[0]), 1, whole, d_one.data_ptr(), cs)
    eng.patterns_quintet_blocks_dev(d_lin.data_ptr(), per_set, whole, d_exp.data_ptr(), cs)
    assert torch.equal(d_exp.sum(dim=0, dtype=torch.int64), d_one[0].to(torch.int64) & 0xFFFFFFFF), "pooled row != expansion"
    del d_one, d_exp
    for B in BLOCKS:
        starts = np.linspace(0, S, B + 1).astype(np.int64)
        chunk = min(Q, OUT_BYTES // (B * 64))
        lchunk = min(P, OUT_BYTES // (B * 64))
        d_rows = torch.empty((max(chunk, lchunk), B, 16), dtype=torch.int32, device="cuda")

        def five():
            for q0 in range(0, Q, chunk):
                eng.patterns_quintet_blocks_species_dev(d_sets.data_ptr() + 20 * q0, min(chunk, Q - q0), starts,
                                                        d_rows.data_ptr(), cs)

        def four():
            for q0 in range(0, Q, chunk):
                eng.patterns_blocks_species_dev(d_sets4.data_ptr() + 16 * q0, min(chunk, Q - q0), starts, d_rows.data_ptr(), cs)

        def expansion():
            for q0 in range(0, P, lchunk):
                eng.patterns_quintet_blocks_dev(d_lin.data_ptr() + 20 * q0, min(lchunk, P - q0), starts, d_rows.data_ptr(), cs)

        ms = timed_in_turns(torch, dict(five=five, four=four, expansion=expansion), reps)
        res[f"quintet_blocks_species_B{B}_ms"] = round(ms["five"], 4)
        res[f"blocks_species_B{B}_ms"] = round(ms["four"], 4)
        res[f"expansion_B{B}_sample_ms"] = round(ms["expansion"], 4)
        res[f"expansion_B{B}_scaled_ms"] = round(ms["expansion"] * Q / len(pick), 3)
        del d_rows
    return res


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 7
    res = dict(tool="species_quintet_bench", reps=reps, S=S, expansion="timed on the sample, scaled to all sets", shapes=[])
    for K, n_per in SHAPES:
        inputs = shape_inputs(K, n_per)
        with QuartetEngine(0) as eng:
            res["shapes"].append(bench_shape(eng, K, n_per, reps, inputs))
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
