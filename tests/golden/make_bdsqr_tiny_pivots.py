"""Writes tests/golden/bdsqr_tiny_pivots.npz: what tq_bdsqr_kernel gives on the bidiagonals of
test_gpu_svd_rare_paths.tiny_pivot_bidiagonals(), each alone in a wave of 64 copies of itself (needs a GPU).

The fixture has to come from a kernel that clamps and selects in EVERY rotation step -- the form before the guards moved
to a cold branch (commit e8f9cf1) -- so build the library from that commit and point TQ_LIB_PATH at it:

    TQ_LIB_PATH=/path/to/libtetrad_hip_e8f9cf1.so python tests/golden/make_bdsqr_tiny_pivots.py [OUT.npz]
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parents[1])]

from test_gpu_svd_rare_paths import GOLDEN_TINY, WAVE, tiny_pivot_bidiagonals  # noqa: E402
from tetrad_amd.engine import QuartetEngine  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN_TINY
de = tiny_pivot_bidiagonals()
sv, steps, sweeps = [], [], []
with QuartetEngine(0) as eng:
    for i in range(len(de)):
        s, st, sw, _ = eng.debug_bdsqr(np.repeat(de[i:i + 1], WAVE, axis=0), reps=1)
        assert (s.view(np.uint64) == s[0].view(np.uint64)).all() and (st == st[0]).all() and (sw == sw[0]).all()
        sv.append(s[0]); steps.append(st[0]); sweeps.append(sw[0])
out.parent.mkdir(parents=True, exist_ok=True)
np.savez(out, de=de, sv=np.stack(sv), steps=np.array(steps, np.uint32), sweeps=np.array(sweeps, np.uint32),
         kernel_commit=np.array("e8f9cf1"))
print(f"wrote {out}: steps {steps}, sweeps {sweeps}")
