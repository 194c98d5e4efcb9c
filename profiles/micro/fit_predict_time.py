"""Diagnostic (not part of the product): cost of predicting at new locations during the fit (stm_mcmc_points,
predict.fit_predict) at config #3's tree, against the same fit without points.  New points: a side x side grid offset by half
a grid step.  Every iteration is saved (burn 0, thin 1), so fit milliseconds per iteration = per saved iteration; the chain is
the same in every variant, so the differences are the prediction alone.
    python profiles/micro/fit_predict_time.py [side] [keep] [grid_side]        timing of every variant, then peak host memory
    python profiles/micro/fit_predict_time.py --mem VARIANT [side] [keep] [grid_side]   one variant, peak host memory (child)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import fit  # noqa: E402
from spamtree_amd.predict import fit_predict  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402

QS = (0.025, 0.5, 0.975)
VARIANTS = {   # name: (points, new_draws, quantiles, save_w / save_yhat)
    "no points": (False, False, (), False),
    "summaries only": (True, False, (), False),
    "summaries + quantile storage": (True, False, QS, False),
    "draws copied to the host": (True, True, (), False),
    "no points, save_w": (False, False, (), True),
    "summaries only, save_w": (True, False, (), True),
}


def run(wl, pts, Xn, name, keep):
    points, draws, qs, save = VARIANTS[name]
    kw = dict(mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=save, save_yhat=save)
    t0 = time.perf_counter()
    if points:
        out = fit_predict(wl, pts, np.ones(pts.shape[0], dtype=np.int64), Xn, quantiles=qs, return_draws=draws, **kw)
    else:
        k = wl["theta"].size
        out = fit.spamtree_mv_mcmc(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"],
                                   wl["res_is_ref"], wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"],
                                   wl["indexing"], wl["bounds"], np.zeros((wl["n"], 1)), wl["theta"], np.zeros(wl["p"]), 0.1,
                                   0.01 * np.eye(k), **kw)
    wall = time.perf_counter() - t0
    return out, dict(variant=name, ms_per_saved_iter=1e3 * out["mcmc_time"] / keep, wall_s=wall,
                     routes=out["new"]["route"] if points else [], accepted=len({tuple(c) for c in out["theta_mcmc"].T}))


def peak_rss_mb():
    """VmHWM: the peak resident set of this process image (ru_maxrss would carry over the parent's peak across fork + exec)."""
    for line in open("/proc/self/status"):
        if line.startswith("VmHWM:"):
            return int(line.split()[1]) / 1024.0
    return float("nan")


def setup(side, grid_side):
    wl = make_workload(side, device=0)
    g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    Xn = np.random.default_rng(3).standard_normal((pts.shape[0], wl["p"]))
    return wl, pts, Xn


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--mem" in sys.argv:
        name, rest = args[0], args[1:]
    else:
        name, rest = None, args
    side = int(rest[0]) if len(rest) > 0 else 1000
    keep = int(rest[1]) if len(rest) > 1 else 50
    grid_side = int(rest[2]) if len(rest) > 2 else 1000
    if name is not None:
        wl, pts, Xn = setup(side, grid_side)
        rss0 = peak_rss_mb()
        _, r = run(wl, pts, Xn, name, keep)
        r["peak_rss_MB"] = peak_rss_mb()
        r["peak_rss_before_fit_MB"] = rss0
        print(json.dumps(r))
        return
    wl, pts, Xn = setup(side, grid_side)
    print(f"n = {wl['n']}, {pts.shape[0]} new points (grid {grid_side}^2 offset by half a step), keep {keep}", flush=True)
    run(wl, pts, Xn, "no points", 3)          # warm-up: code objects, allocations
    for name in VARIANTS:
        if not VARIANTS[name][3]:
            print(json.dumps(run(wl, pts, Xn, name, keep)[1]), flush=True)
    for name in ("no points, save_w", "summaries only, save_w", "summaries only", "draws copied to the host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mem", name, str(side), str(keep), str(grid_side)],
                           capture_output=True, text=True, timeout=900)
        print(r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else f"{name}: failed ({r.returncode}) {r.stderr[-400:]}",
              flush=True)
        if r.returncode != 0:
            break


if __name__ == "__main__":
    main()
