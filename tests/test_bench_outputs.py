"""bench.py's plain run and `--dump-outputs`: the rows the last timed step delivered, written as float .npy files
(CPU: the writer and its size cap; GPU: a plain run's line and its rows against the engine's own answer)."""
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module_outputs", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["bench_module_outputs"] = mod
    spec.loader.exec_module(mod)
    return mod


def test_full_is_off_by_default_and_subsample_mode_has_its_own_switch():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.no_subsample, a.dump_outputs, a.steps, a.warmup) == (False, False, None, 7, 2)
    a = bench.parse_args(["--full", "--no-subsample", "--dump-outputs", "d"])
    assert (a.full, a.no_subsample, a.dump_outputs) == (True, True, "d")


def test_dump_writes_every_row_exactly_in_float(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(1)
    Q = 1000
    rstat = rng.integers(0, 2 ** 32, size=(Q, 2), dtype=np.uint32)
    rscor = rng.standard_normal((Q, 3))
    flags = rng.integers(0, 32, size=Q, dtype=np.uint8)
    bench.dump_outputs(tmp_path / "out", rstat, rscor, flags)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert sorted(got) == ["flags", "rscor", "rstat"]
    assert got["rstat"].dtype == np.float64 and got["rscor"].dtype == np.float64 and got["flags"].dtype == np.float32
    np.testing.assert_array_equal(got["rstat"].astype(np.uint32), rstat)
    np.testing.assert_array_equal(got["rscor"], rscor)
    np.testing.assert_array_equal(got["flags"].astype(np.uint8), flags)


def test_dump_of_a_large_batch_is_a_fixed_sample_under_64_mb(tmp_path):
    bench = _bench()
    Q = 2_000_000                               # 88 MB of rows in float
    rstat = np.stack([np.arange(Q), np.arange(Q) * 3], axis=1).astype(np.uint32)
    rscor = np.arange(3 * Q, dtype=np.float64).reshape(Q, 3)
    flags = (np.arange(Q) % 7).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, rstat, rscor, flags)
    total = sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy"))
    assert total <= 64 * 10 ** 6
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))     # the same sample every time
    idx = rows.astype(np.int64)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rstat.npy"), rstat[idx].astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "rscor.npy"), rscor[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "flags.npy"), flags[idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_timed_rows(tmp_path):
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    Q = 20000
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--quartets", str(Q), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "quartets/s" and d["higher_is_better"] is True and d["metric"] and d["dtype"]
    assert "roofline" not in d and "cpu_baseline" not in d and "full_mode_value" not in d     # those are --full's
    got = {name: np.load(tmp_path / f"{name}.npy") for name in ("rstat", "rscor", "flags")}
    assert got["rstat"].shape == (Q, 2) and got["rscor"].shape == (Q, 3) and got["flags"].shape == (Q,)
    # the benchmark's input, rebuilt from its seeds, through the host-buffer API
    T, S, _ = synth.CONFIGS["c3"]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS["c3"])
    ranks = np.random.default_rng(synth.CONFIG_SEEDS["c3"] + 1000).choice(synth.comb(T, 4), size=Q, replace=False)
    with QuartetEngine(0) as eng:
        eng.set_data(tmparr, tmpmap)
        rstat, rscor, flags = eng.resolve(synth.unrank_quartets(ranks, T), True)
    np.testing.assert_array_equal(got["rstat"], rstat.astype(np.float64))
    np.testing.assert_array_equal(got["rscor"], rscor)
    np.testing.assert_array_equal(got["flags"], flags.astype(np.float32))
