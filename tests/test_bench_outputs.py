"""bench.py --dump-outputs: what the last timed step computed, as .npy files within a size budget, identical from run to run;
--steps sets the number of timed steps and the result line carries ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)


def run(args, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)


def test_dump_within_budget_writes_everything(tmp_path):
    import bench
    out = {"theta": np.array([2.3, 1.0, 1.0, 6.0]), "Bcoeff": np.arange(6.0).reshape(3, 2), "w": np.linspace(-1, 1, 1000)}
    bench.dump_outputs(out, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["Bcoeff.npy", "theta.npy", "w.npy"]
    for k, v in out.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, v)


def test_dump_over_budget_samples_the_largest_array_the_same_way_every_time(tmp_path):
    import bench
    rng = np.random.default_rng(5)
    out = {"loglik": np.array([-1022.3]), "w": rng.standard_normal(50_000)}
    budget = 100_000                                             # w alone is 400 kB
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d), budget=budget)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= budget
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["loglik.npy", "w.npy", "w_index.npy"]
    idx = np.load(a / "w_index.npy")
    assert idx.dtype == np.float64 and idx.size > 1000 and np.all(np.diff(idx) > 0)
    w = np.load(a / "w.npy")
    assert np.array_equal(w, out["w"][idx.astype(np.int64)])
    assert np.array_equal(np.load(b / "w_index.npy"), idx) and np.array_equal(np.load(b / "w.npy"), w)
    assert np.array_equal(np.load(a / "loglik.npy"), out["loglik"])


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_validated(args):
    r = run(args + ["--launch-check"], timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


@pytest.mark.gpu
def test_dump_outputs_are_the_last_timed_step_and_repeat_exactly(tmp_path):
    steps, warmup = 3, 2
    lines = []
    for d in ("a", "b"):
        r = run(["--side", "60", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--stationary-windows", "0",
                 "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    for res in lines:
        assert res["steps"] == steps and res["ms_per_step"] > 0
        assert abs(res["ms_per_step"] * res["value"] - 1e3) < 1e-6 * 1e3
    a, b = tmp_path / "a", tmp_path / "b"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"w.npy", "theta.npy", "Bcoeff.npy", "tausq_inv.npy", "loglik.npy", "iteration.npy"} <= set(names)
    assert np.load(a / "iteration.npy")[0] == warmup + steps           # the untimed passes after the timed steps are not in it
    assert np.load(a / "w.npy").shape == (lines[0]["config"]["n"],)
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x))
        assert np.array_equal(x, y), f
