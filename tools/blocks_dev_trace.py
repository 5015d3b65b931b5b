"""Five tq_patterns_blocks_dev calls back to back on one stream (more calls than staging pieces), for a count of the HIP
calls of that path under `rocprofv3 --hip-trace --stats`.   python tools/blocks_dev_trace.py"""
import sys
from pathlib import Path; sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
from tetrad_amd import synth
from tetrad_amd.engine import QuartetEngine
T, S = 12, 4101
tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=71, missing=0.15)
sets = np.ascontiguousarray(synth.all_quartets(T)[:20], dtype=np.uint32)
starts = [[3, 2047, 2060, S], [0, S], [1, 40, 2048, 2081, S - 1], [2043, 2053, S], [0, 31, 64, 4096]]
eng = QuartetEngine(0); eng.set_data(tmparr, tmpmap)
d_sets = torch.from_numpy(sets.view(np.int32)).cuda()
outs = [torch.zeros((len(sets), len(b) - 1, 16), dtype=torch.int32, device="cuda") for b in starts]
stream = torch.cuda.Stream()
torch.cuda.synchronize()
for b, out in zip(starts, outs):
    eng.patterns_blocks_dev(d_sets.data_ptr(), len(sets), b, out.data_ptr(), stream.cuda_stream)
torch.cuda.synchronize()
print("block rows:", [int(o[:, :, 15].sum()) for o in outs])
eng.close()
