"""bench.py's command line: a plain run carries the headline figure only, `--full` the rest, `--dump-outputs DIR`
writes what the last timed step returned, and `--steps` is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _line(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_writes_float64_and_samples_what_exceeds_the_budget(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    big = np.arange(300_000, dtype=np.float64)
    outputs = {"value": [1.5], "index": np.array([7], dtype=np.int64), "big": big}
    bench.dump_outputs(str(tmp_path), outputs)
    assert np.load(tmp_path / "value.npy").tolist() == [1.5]
    idx = np.load(tmp_path / "index.npy")
    assert idx.dtype == np.float64 and idx.tolist() == [7.0]
    sample, where = np.load(tmp_path / "big.npy"), np.load(tmp_path / "big_sample_index.npy")
    assert sample.dtype == np.float64 and sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 1 << 20
    np.testing.assert_array_equal(sample, big[where.astype(np.int64)])
    again = tmp_path / "again"
    bench.dump_outputs(str(again), outputs)  # a fixed sample: two builds compare element for element
    np.testing.assert_array_equal(np.load(again / "big_sample_index.npy"), where)


def test_bench_refuses_zero_timed_steps():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be >= 1" in (r.stdout + r.stderr)


@pytest.mark.gpu
def test_plain_run_times_the_steps_it_was_given_and_dumps_the_last_step(tmp_path):
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c4", "--m-per-gpu", "2000"]
    outs = []
    for k in range(2):
        out = _line(_run(common + ["--dump-outputs", str(tmp_path / str(k))]))
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        for key in ("metric", "unit", "higher_is_better", "dtype"):
            assert key in out
        assert "secondary" not in out and "cpu_baseline" not in out and "update_ms" not in out["config"]
        outs.append(out)
    d0, d1 = tmp_path / "0", tmp_path / "1"
    assert sorted(os.listdir(d0)) == ["qei_values.npy", "winner_index.npy", "winner_value.npy"]
    vals = np.load(d0 / "qei_values.npy")
    assert vals.dtype == np.float64 and vals.shape == (2000,)
    assert np.load(d0 / "winner_value.npy")[0] == vals.max() == outs[0]["config"]["best_value"]
    assert np.load(d0 / "winner_index.npy")[0] == np.argmax(vals) == outs[0]["config"]["best_index"]
    for name in os.listdir(d0):  # same arguments, same inputs, same outputs
        np.testing.assert_array_equal(np.load(d0 / name), np.load(d1 / name))


@pytest.mark.gpu
def test_full_run_adds_the_informational_figures():
    out = _line(_run(["--gpus", "1", "--steps", "1", "--warmup", "0", "--workload", "c2", "--m-per-gpu", "20000",
                      "--full", "--no-cpu-baseline"]))
    assert out["config"]["update_ms"] > 0
    assert isinstance(out["config"]["acquire_ms"], float) and isinstance(out["config"]["fit"], dict)
