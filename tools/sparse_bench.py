"""Subsample-mode throughput of tq_resolve_to_host on a c3-shaped matrix of one profile: 1e6 random quartets on the device,
rows to pinned host arrays (the path bench.py times), plus the duration of tq_set_data.  One JSON line.

  python tools/sparse_bench.py [rad30|rad60|rad85|c3] [--steps K] [--warmup W] [name=value ...]      (engine options)

The sparse leg of the no-regression check of option site_pack: on rad60 the automatic rule must keep the natural layout, so
the figure must not move against a build without the option (profiles/site_pack/README.md)."""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from tetrad_amd import synth
from tetrad_amd.engine import QuartetEngine, pinned_empty


def main(argv):
    profile, steps, warmup, opts = "rad60", 10, 2, {}
    it = iter(argv)
    for a in it:
        if a == "--steps":
            steps = int(next(it))
        elif a == "--warmup":
            warmup = int(next(it))
        elif "=" in a:
            k, v = a.split("=")
            opts[k] = int(v)
        else:
            profile = a
    T, S, Q = synth.CONFIGS["c3"]
    if profile == "c3":
        tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS["c3"])
    else:
        tmparr, tmpmap = synth.radseq_profile(profile)
    q = synth.random_quartets(T, Q, seed=4242)
    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(q.astype(np.int32)).to(dev)
    out = (pinned_empty((Q, 2), np.uint32), pinned_empty((Q, 3), np.float64), pinned_empty(Q, np.uint8))
    with QuartetEngine(0) as eng:
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.set_data(tmparr, tmpmap)
        t_set = []
        for _ in range(5):
            t0 = time.perf_counter()
            eng.set_data(tmparr, tmpmap)
            t_set.append(time.perf_counter() - t0)
        for _ in range(warmup):
            eng.resolve_to_host(d_q.data_ptr(), Q, True, out=out)
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            eng.resolve_to_host(d_q.data_ptr(), Q, True, out=out)
            ts.append(time.perf_counter() - t0)
        state = eng.site_pack_state() if hasattr(eng, "site_pack_state") else None
    ms = np.array(ts) * 1e3
    print(json.dumps(dict(profile=profile, quartets=Q, options=opts, steps=steps, ms_per_step_mean=round(float(ms.mean()), 4),
                          ms_per_step_min=round(float(ms.min()), 4), mquartets_per_s=round(Q / float(ms.mean()) / 1e3, 3),
                          nsnps_sum=int(out[0][:, 1].astype(np.int64).sum()), set_data_ms_min=round(min(t_set) * 1e3, 3),
                          set_data_ms_median=round(float(np.median(t_set)) * 1e3, 3), packed_sites_and_in_use=state)))


if __name__ == "__main__":
    main(sys.argv[1:])
