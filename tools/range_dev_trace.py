"""Five tq_resolve_range_dev calls without a quartet array back to back on one stream (the already-ordered path of the stream
rule: no wait is due), for a count of the HIP calls of that path under `rocprofv3 --hip-trace --stats`.
python tools/range_dev_trace.py"""
import sys
from pathlib import Path; sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from tetrad_amd import synth
from tetrad_amd.engine import QuartetEngine
T, S, Q = 16, 4101, 1000
tmparr, tmpmap = synth.simulate_tmparr(T, S, seed=81, missing=0.15)
eng = QuartetEngine(0); eng.set_data(tmparr, tmpmap)
outs = [(torch.zeros((Q, 2), dtype=torch.int32, device="cuda"), torch.zeros((Q, 3), dtype=torch.float64, device="cuda"),
         torch.zeros(Q, dtype=torch.uint8, device="cuda")) for _ in range(5)]
stream = torch.cuda.Stream()
torch.cuda.synchronize()
for i, (rstat, rscor, flags) in enumerate(outs):
    eng.resolve_range_dev(160 * i, Q, i % 2 == 0, 0, rstat.data_ptr(), rscor.data_ptr(), flags.data_ptr(), stream.cuda_stream)
torch.cuda.synchronize()
print("counted sites:", [int(o[0][:, 1].sum()) for o in outs])
eng.close()
