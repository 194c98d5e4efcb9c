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


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_untimed_figures_after_the_same_step(tmp_path):
    """A plain run prints the headline figures of its timed steps and nothing that takes runs of its own; --full adds the
    per-launch phase pass, the measured peaks and the stationary windows, after the dump: the dumped step is the same."""
    common = ["--side", "60", "--steps", "3", "--warmup", "2"]
    r = run(common + ["--dump-outputs", str(tmp_path / "plain")])
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    r = run(common + ["--full", "--no-cpu-baseline", "--stationary-windows", "1", "--dump-outputs", str(tmp_path / "full")])
    assert r.returncode == 0, r.stderr[-2000:]
    full = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for res in (plain, full):
        assert res["unit"] == "Gibbs iterations/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
        assert res["metric"].startswith("Gibbs iterations/sec") and res["steps"] == 3 and res["warmup"] == 2
        assert abs(res["ms_per_step"] * res["value"] - 1e3) < 1e-6 * 1e3
        assert res["roofline"]["achieved"] > 0 and res["roofline"]["fp64_pipe"]["achieved"] > 0
    assert not {"stationary", "cpu_baseline"} & set(plain)
    assert not {"by_level_ms", "sample_by_level_ms", "phase_ms_per_iter", "peak_measured", "all_levels"} & set(plain["roofline"])
    assert "cpu_baseline" not in full and full["stationary"]["windows"]
    rf = full["roofline"]
    assert len(rf["by_level_ms"]) == full["config"]["levels"] == plain["config"]["levels"]
    assert {"factor", "sample", "loglik"} <= set(rf["phase_ms_per_iter"]) and "stream_copy_GBps" in rf["peak_measured"]
    assert rf["algorithmic_bytes_per_launch"] == plain["roofline"]["algorithmic_bytes_per_launch"]
    a, b = tmp_path / "plain", tmp_path / "full"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and np.load(a / "iteration.npy")[0] == 2 + 3
    for f in names:
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
