"""Diagnostic (not part of the product): cost of the Rao-Blackwellised exceedance probabilities at new points (st_points_exceed_*,
predict.fit_predict(exceed=)) at config #3's tree, against the same fit_predict without `exceed` (no exceedance step runs, nothing
is allocated for it).  New points: the side x side grid offset by half a grid step, with regressors, so both
targets (w and yhat) are accumulated.  Summaries only, nothing saved per draw; every iteration is saved (burn 0, thin 1), so fit
milliseconds per iteration = per saved iteration.  The three variants -- without, T = 1, T = 8 -- alternate, `rounds` times each;
the chain and the predictive means must be identical in all of them.
    python profiles/micro/exceed_time.py [side] [keep] [grid_side] [rounds]
Then, or alone with `launches` as the first argument, on a handle of its own: `reps` calls of st_points_accumulate with T thresholds
set (T = 0: none), device-synchronised wall time per call, and the copy bandwidth st_probe_peaks measures in the same run -- under
`rocprofv3 --kernel-trace --stats` this is the run whose k_exceed_acc rows belong to one T.
    python profiles/micro/exceed_time.py launches [side] [grid_side] [T] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import SpamTreeMV, _dp  # noqa: E402
from spamtree_amd.predict import fit_predict, locate  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402

SIDES8 = [1, -1, 1, -1, 1, -1, 1, -1]
THR8 = [float(x) for x in np.linspace(-1.5, 1.5, 8)]
SPECS = {0: None, 1: dict(thresholds=THR8[3:4], side=SIDES8[:1]), 8: dict(thresholds=THR8, side=SIDES8)}


def setup(side, grid_side):
    wl = make_workload(side, device=0)
    g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    Xn = np.random.default_rng(3).standard_normal((pts.shape[0], wl["p"]))
    return wl, pts, Xn


def model_bytes(n, p, T, targets=2):
    """Per point 20 + 8 p B of inputs (cond_mean, cond_var, the margin, p regressors), per target 16 T B of state read and written."""
    return float(n) * (20 + 8 * p + targets * 2 * 16 * T)


def run(wl, pts, Xn, T, keep):
    out = fit_predict(wl, pts, np.ones(pts.shape[0], dtype=np.int64), Xn, return_draws=False, exceed=SPECS[T], mcmc_keep=keep,
                      mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False, save_yhat=False)
    return out, 1e3 * out["mcmc_time"] / keep


def fits(wl, pts, Xn, keep, rounds):
    for T in SPECS:                                         # warm-up: code objects, allocations
        run(wl, pts, Xn, T, 3)
    ms = {T: [] for T in SPECS}
    last = {}
    for _ in range(rounds):
        for T in SPECS:
            last[T], t = run(wl, pts, Xn, T, keep)
            ms[T].append(t)
        for T in (1, 8):                                    # the chain and the predictive means, bit for bit
            for key in ("theta_mcmc", "beta_mcmc", "tausq_mcmc"):
                assert np.array_equal(last[0][key], last[T][key]), (T, key)
            for key in ("mean", "var", "w_mean", "yhat_mean"):
                assert np.array_equal(last[0]["new"][key], last[T]["new"][key]), (T, key)
    res = dict(ms_per_saved_iter={f"T{T}": v for T, v in ms.items()})
    for T in (1, 8):
        ex = last[T]["new"]["exceed"]
        res[f"T{T}"] = dict(added_ms_median=float(np.median(np.array(ms[T]) - np.array(ms[0]))), spread_ms=float(max(ms[T]) - min(ms[T])),
                            n_accumulated=ex["n_accumulated"], mean_prob_w=ex["w"]["prob"].mean(axis=1).tolist(),
                            mean_prob_yhat=ex["yhat"]["prob"].mean(axis=1).tolist(), max_prob_var=float(ex["w"]["prob_var"].max()),
                            model_bytes=model_bytes(pts.shape[0], int(wl["p"]), T))
    res["spread_without_ms"] = float(max(ms[0]) - min(ms[0]))
    res["accepted"] = len({tuple(c) for c in last[0]["theta_mcmc"].T})
    return res


def launches(wl, pts, Xn, T, reps):
    """`reps` device-synchronised st_points_accumulate calls with T thresholds set (0: none) on one state, ms per call, and the copy
    bandwidth of the same run."""
    mv = np.ones(pts.shape[0], dtype=np.int64)
    p = int(wl["p"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.zeros(int(wl["n"])), np.zeros(p), wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    hm.set_points(pts, mv, locate(wl["topo"], pts, mv, device=0), Xn)
    if T:
        hm.set_exceed(SPECS[T]["thresholds"], SPECS[T]["side"])
    ts = []
    for s in range(reps + 2):
        hm.synchronize()
        t0 = time.perf_counter()
        hm._check(hm.lib.st_points_accumulate(hm.h, 11, s, None, None, None, None))
        hm.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    peaks = np.zeros(3)
    hm._check(hm.lib.st_probe_peaks(0, 1 << 30, 5, _dp(peaks)))
    res = dict(T=T, reps=reps, accumulate_ms_median=float(np.median(ts[2:])), accumulate_ms_min=float(min(ts[2:])), copy_GBps=float(peaks[0]),
               model_bytes=model_bytes(pts.shape[0], p, T) if T else 0.0)
    if T:
        res["model_us_at_copy_bandwidth"] = res["model_bytes"] / (peaks[0] * 1e9) * 1e6
        res["mean_prob_w"] = hm.exceed()["w"]["prob"].mean(axis=1).tolist()
    hm.close()
    return res


def main():
    if sys.argv[1:2] == ["launches"]:
        a = [int(x) for x in sys.argv[2:]]
        side, grid_side, T, reps = (a + [1000, 1000, 8, 20][len(a):])[:4]
        wl, pts, Xn = setup(side, grid_side)
        print(json.dumps(dict(new_points=pts.shape[0], launches=launches(wl, pts, Xn, T, reps))), flush=True)
        return
    a = [int(x) for x in sys.argv[1:]]
    side, keep, grid_side, rounds = (a + [1000, 50, 1000, 3][len(a):])[:4]
    wl, pts, Xn = setup(side, grid_side)
    print(f"n = {wl['n']}, {pts.shape[0]} new points, p = {wl['p']}, keep {keep}", flush=True)
    res = dict(new_points=pts.shape[0], keep=keep, fit=fits(wl, pts, Xn, keep, rounds))
    print(json.dumps(res["fit"]), flush=True)
    res["launches"] = [launches(wl, pts, Xn, T, 20) for T in (0, 1, 8)]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
