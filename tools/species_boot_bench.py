#!/usr/bin/env python
"""Time the bootstrap loop for species trees (`species.bootstrap_species_trees`).

Shape: K = 32 species x 4 samples (T = 128), S = 50 000 source sites with 15 % two-base codes, all 35 960 species
quartets, option "species_alleles" on.
  1. replicates per second of the whole loop (draws, replicate build, species table, pooled counts, singular values,
     exact supertree), for `supertree="device"` and `"host"` (wall time of `nboots` replicates after one warm-up run);
  2. the allele table build (`tq_species_allele_table_kernel`) alone: the "order" slot of `timing_read_kernels` of a
     species call right after a new replicate (median of `reps`), next to the lineage table build on the same replicate.

    python tools/species_boot_bench.py [nboots] [reps] [--out FILE]
Prints one JSON line (and writes it to FILE)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tetrad_amd import species, synth  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

K, N, S = 32, 4, 50_000


def table_ms(eng, rows, lidxs, alleles, reps):
    out = []
    for r in range(reps):
        eng.bootstrap(lidxs, r, r)                                    # a new replicate: the next call rebuilds the table
        eng.set_option("species_alleles", alleles)
        eng.timing_read_kernels()
        eng.resolve_species(rows)
        k, _ = eng.timing_read_kernels()
        eng.set_option("species_alleles", 0)
        out.append(k["order"])
    return round(float(np.median(out)), 4)


def main():
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    nboots = int(args[0]) if args else 20
    reps = int(args[1]) if len(args) > 1 else 5
    tmparr, tmpmap, sp, _ = synth.simulate_species(K, N, S, seed=103)
    seqarr, _, spans = synth.make_c5_source(source=(tmparr, tmpmap), ambiguous=0.15)
    smap = species.SpeciesMap(sp, [f"sp{k:02d}" for k in range(K)])
    res = dict(tool="species_boot_bench", K=K, samples_per_species=N, S0=S, nloci=int(spans.shape[0]),
               species_quartets=35_960, nboots=nboots, reps=reps)
    with QuartetEngine(0) as eng:
        for back in ("device", "host"):
            species.bootstrap_species_trees(eng, seqarr, spans, smap, 2, seed=1, supertree=back)        # warm-up
            t0 = time.perf_counter()
            trees = species.bootstrap_species_trees(eng, seqarr, spans, smap, nboots, seed=2, supertree=back)
            dt = time.perf_counter() - t0
            res[f"replicates_per_s_{back}"] = round(len(trees) / dt, 2)
            res[f"ms_per_replicate_{back}"] = round(1e3 * dt / len(trees), 3)
        rows = species.species_quartets(K)
        lidxs = np.random.default_rng(3).integers(0, spans.shape[0], spans.shape[0])
        eng.timing_enable(True)
        res["allele_table_ms"] = table_ms(eng, rows, lidxs, 1, reps)
        res["lineage_table_ms"] = table_ms(eng, rows, lidxs, 0, reps)
        eng.timing_enable(False)
    line = json.dumps(res)
    print(line)
    if out:
        Path(out).write_text(line + "\n")


if __name__ == "__main__":
    main()
