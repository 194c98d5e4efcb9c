"""Diagnostic (not part of the product): cost of the mixture predictive at new points (st_points_mixture_*, predict.fit_predict(mixture=))
at config #3's tree.  New points: the side x side grid offset by half a grid step, with regressors.
    python profiles/micro/mixture_time.py [side] [keep] [grid_side] [rounds]
fit_predict with `mixture=dict(probs=[0.025, 0.5, 0.975])` against the same call without it (the parent's path: no store, nothing
launched for it), alternating, `rounds` times each; summaries only, every iteration saved (burn 0, thin 1), so fit milliseconds per
iteration = per saved iteration; theta, beta, tausq and the predictive means must be identical.  The read-out after the chain (the
quantile kernel over `keep` components) is outside the driver's clock and reported from the wall clock of the whole call.
    python profiles/micro/mixture_time.py kernels [side] [grid_side] [K] [scored_small] [scored_large]
On a handle of its own: K saved iterations into the store and into the stored draws of st_points_summary_reserve (the same draws), then
one call each of st_points_mixture_quantiles at T = 1 and T = 3 (target w), st_points_mixture_crps with `scored_small` and
`scored_large` scored points, and for context st_points_summary_quantile and the stored-draw CRPS of st_points_score_get on the
same points; device-synchronised wall time per call (it includes the copy of the results), the passes per quantile from
st_points_mixture_info, and the FP64 vector (v_fma_f64) rate and copy bandwidth st_probe_peaks measures in the same run.  Under
`rocprofv3 --kernel-trace --stats` the kernel rows of this run are the kernels' own times, in this order of calls."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib  # noqa: E402
from spamtree_amd.model import SpamTreeMV, _dp  # noqa: E402
from spamtree_amd.predict import fit_predict, locate  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402

PROBS3 = [0.025, 0.5, 0.975]


def setup(side, grid_side):
    wl = make_workload(side, device=0)
    g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    Xn = np.random.default_rng(3).standard_normal((pts.shape[0], wl["p"]))
    return wl, pts, Xn


def run(wl, pts, Xn, mix, keep):
    t0 = time.perf_counter()
    out = fit_predict(wl, pts, np.ones(pts.shape[0], dtype=np.int64), Xn, return_draws=False, mixture=dict(probs=PROBS3) if mix else None,
                      mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False, save_yhat=False)
    return out, 1e3 * out["mcmc_time"] / keep, time.perf_counter() - t0


def fits(wl, pts, Xn, keep, rounds):
    for mix in (False, True):                               # warm-up: code objects, allocations
        run(wl, pts, Xn, mix, 3)
    ms, wall, last = {False: [], True: []}, {False: [], True: []}, {}
    for _ in range(rounds):
        for mix in (False, True):
            last[mix], t, w = run(wl, pts, Xn, mix, keep)
            ms[mix].append(t)
            wall[mix].append(w)
        for key in ("theta_mcmc", "beta_mcmc", "tausq_mcmc"):   # the chain and the predictive means, bit for bit
            assert np.array_equal(last[False][key], last[True][key]), key
        for key in ("mean", "var", "w_mean", "yhat_mean"):
            assert np.array_equal(last[False]["new"][key], last[True]["new"][key]), key
    mq = last[True]["new"]["mixture"]
    return dict(ms_per_saved_iter=dict(without=ms[False], mixture=ms[True]), wall_s=dict(without=wall[False], mixture=wall[True]),
                added_ms_median=float(np.median(np.array(ms[True]) - np.array(ms[False]))),
                spread_ms=dict(without=float(max(ms[False]) - min(ms[False])), mixture=float(max(ms[True]) - min(ms[True]))),
                store_bytes_per_saved_iter=24.0 * pts.shape[0], n_stored=mq["n_stored"], n_unconverged=mq["n_unconverged"],
                mean_width_95_yhat=float(np.mean(mq["yhat"][2] - mq["yhat"][0])), accepted=len({tuple(c) for c in last[False]["theta_mcmc"].T}))


def timed(hm, call):
    hm.synchronize()
    t0 = time.perf_counter()
    res = call()
    hm.synchronize()
    return res, 1e3 * (time.perf_counter() - t0)


def kernels(wl, pts, Xn, K, scored):
    n = pts.shape[0]
    mv = np.ones(n, dtype=np.int64)
    p = int(wl["p"])
    rng = np.random.default_rng(5)
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    rng.standard_normal(int(wl["n"])), 0.1 * rng.standard_normal(p), wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    hm.set_points(pts, mv, locate(wl["topo"], pts, mv, device=0), Xn)
    ys = {}
    for m in scored:
        y = np.full(n, np.nan)
        idx = rng.choice(n, size=m, replace=False)
        y[idx] = rng.standard_normal(m)
        ys[m] = y
    hm.reserve_mixture(K)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, K))
    hm._check(hm.lib.st_points_summary_reset(hm.h))
    ts = []
    for s in range(K):                                      # K components that differ: another w (a scaled copy) every few draws
        if s % 50 == 0:
            hm.set_w(rng.standard_normal(int(wl["n"])))
        _, t = timed(hm, lambda: hm._check(hm.lib.st_points_accumulate(hm.h, 11, s, None, None, None, None)))
        ts.append(t)
    res = dict(K=K, new_points=n, accumulate_ms_median=float(np.median(ts[2:])), info=hm.mixture_info())
    q1 = np.zeros((1, n)); q3 = np.zeros((3, n))
    for name, probs, buf in (("quantile_T1", [0.5], q1), ("quantile_T3", PROBS3, q3)):
        pr = np.array(probs)
        unc = C.c_int64()
        out = _lib.StMixOut(_dp(buf), C.pointer(unc))
        _, t = timed(hm, lambda: hm._check(hm.lib.st_points_mixture_quantiles(hm.h, pr.size, _dp(pr), C.byref(out), None, None)))
        info = hm.mixture_info()
        res[name] = dict(ms=t, n_unconverged=int(unc.value), passes_per_quantile=info["n_passes"] / max(info["n_solved"], 1))
    a = np.zeros(n)
    _, t = timed(hm, lambda: hm._check(hm.lib.st_points_summary_quantile(hm.h, 0.5, _dp(a), None)))
    res["stored_draw_quantile_w"] = dict(ms=t, mean_abs_gap_to_mixture_median=float(np.mean(np.abs(a - q1[0]))))
    for m in scored:
        hm.set_scores(ys[m])
        hm.accumulate_points(seed=11, it=0)                 # the scores want an iteration of their own; the full stores take no more
        mc, t = timed(hm, hm.mixture_crps)
        sc, t2 = timed(hm, lambda: hm.scores(crps=True))
        obs = ~np.isnan(ys[m])
        res[f"crps_{m}"] = dict(ms=t, pairs=0.5 * K * (K - 1) * m, pairs_per_s=0.5 * K * (K - 1) * m / (t * 1e-3), stored_draw_scores_ms=t2,
                                mean_crps_mixture=float(np.mean(mc["crps"][obs])), mean_crps_stored_draws=float(np.mean(sc["crps"][obs])),
                                mean_spread=float(np.mean(mc["spread"][obs])))
    peaks = np.zeros(3)
    hm._check(hm.lib.st_probe_peaks(0, 1 << 30, 5, _dp(peaks)))
    res["peaks"] = dict(copy_GBps=float(peaks[0]), fp64_mfma_TFLOPs=float(peaks[1]), fp64_fma_TFLOPs=float(peaks[2]))
    hm.close()
    return res


def main():
    if sys.argv[1:2] == ["kernels"]:
        a = [int(x) for x in sys.argv[2:]]
        side, grid_side, K, m1, m2 = (a + [1000, 1000, 1000, 10000, 100000][len(a):])[:5]
        wl, pts, Xn = setup(side, grid_side)
        print(json.dumps(kernels(wl, pts, Xn, K, (m1, m2))), flush=True)
        return
    a = [int(x) for x in sys.argv[1:]]
    side, keep, grid_side, rounds = (a + [1000, 50, 1000, 3][len(a):])[:4]
    wl, pts, Xn = setup(side, grid_side)
    print(f"n = {wl['n']}, {pts.shape[0]} new points, p = {wl['p']}, keep {keep}", flush=True)
    print(json.dumps(dict(new_points=pts.shape[0], keep=keep, fit=fits(wl, pts, Xn, keep, rounds))), flush=True)


if __name__ == "__main__":
    main()
