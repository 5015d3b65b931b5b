"""The figures behind PASSES of tests/stream_hold.py (profiles/stream_rule/measure_hold.json): the length of one hold and the
host time to enqueue it, five in a row, and every enqueueing second call of tests/test_gpu_stream_rule.py on an engine that has
made the call before -- alone on an idle device and queued while another stream is held -- with torch timing events recorded
before the Python call and behind it, so the enqueue time is inside.   python tools/stream_hold_measure.py [out.json]"""
import json, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np
import torch
import stream_hold as sh
import test_gpu_stream_rule as tr
from tetrad_amd import synth
from tetrad_amd.engine import QuartetEngine

out = {}
A, B = torch.cuda.Stream(), torch.cuda.Stream()
sh.hold(A); torch.cuda.synchronize()
hold_ms, enq_ms = [], []
for _ in range(5):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record(A); sh.hold(A); e.record(A)
    enq_ms.append((time.perf_counter() - t0) * 1e3)
    e.synchronize(); hold_ms.append(s.elapsed_time(e))
out["hold_ms"] = hold_ms; out["hold_enqueue_ms"] = enq_ms; out["passes"] = sh.PASSES; out["hold_bytes"] = sh.HOLD_BYTES

def time_call(E, c, held=False):
    ms = []
    for _ in range(4):
        torch.cuda.synchronize()
        if held: sh.hold(A)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(B); c.run(E, B.cuda_stream); e.record(B); e.synchronize()
        ms.append(s.elapsed_time(e)); torch.cuda.synchronize()
    return ms[1:]

data = synth.simulate_tmparr(tr.T, tr.S, seed=81, missing=0.15)
calls = {}
with QuartetEngine(0) as E:
    E.set_data(*data); E.set_species(tr.SPECIES_OF_16)
    cs = [tr.range_call(700, 600, True), tr.range_call(700, 600, False), tr.resolve_call(tr.ranks_to_quartets(900, 1700), False),
          tr.resolve_call(tr.ranks_to_quartets(0, 1000)[::-1].copy(), True), tr.species_call(tr.ranks_to_quartets(0, 15, 6)),
          tr.blocks_call("patterns_blocks_dev", tr.ranks_to_quartets(0, 20), tr.STARTS_A), tr.taxon_call(tr.STARTS_A),
          tr.patterns_call(tr.ranks_to_quartets(0, 20), True)] + [tr.caller_memory_call(n)[0] for n in
          ("unrank_dev", "sample_quartets_dev", "dstat_accumulate_dev", "dstat_jackknife_dev", "dstat_jackknife_masks_dev")]
    for c in cs:
        calls[c.name] = {"alone_ms": time_call(E, c), "under_a_hold_ms": time_call(E, c, held=True)}
src = tr.layout_source(10, seed=12); reps = tr.five_draws(src[1], seed=5)
smin = min(int((src[1][r[0], 1] - src[1][r[0], 0]).sum()) for r in reps[:2])
with QuartetEngine(0) as E:
    E.set_option("boot_pack", 1); E.set_source(*src); E.bootstrap(*reps[0][:3]); E.set_species(tr.SPECIES_OF_10)
    for n in tr.CONSUMERS:
        c = tr.consumer(n, smin)
        calls["replicate: " + c.name] = {"alone_ms": time_call(E, c), "under_a_hold_ms": time_call(E, c, held=True)}
out["second_calls"] = calls
out["longest_alone_ms"] = max(max(v["alone_ms"]) for v in calls.values())
out["longest_under_a_hold_ms"] = max(max(v["under_a_hold_ms"]) for v in calls.values())
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps({k: out[k] for k in ("hold_ms", "hold_enqueue_ms", "longest_alone_ms", "longest_under_a_hold_ms")}))
