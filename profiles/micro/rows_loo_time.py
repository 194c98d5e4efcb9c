"""Diagnostic (not part of the product): cost of the leave-one-out criteria with the latent field integrated out
(st_rows_loo_*, stm_mcmc_loo) at config #3's tree (n = 1e6, q = 1, every row observed).
  micro   on a handle of its own: the device-synchronised median of st_rows_loo_accumulate and, beside it in the same run, of
          st_simulate(nd = 1), which reads the same slot-0 panels once from the root down; the copy bandwidth st_probe_peaks measures
          on the same box; st_rows_loo_info's bytes and routes; st_rows_loo_totals once.  Under `rocprofv3 --kernel-trace --stats --
          python ... micro` the trace has the kernels' own times per level.
  fit     fit.spamtree_mv_mcmc(criteria=True, save_w=False, save_yhat=False) with and without loo=True, alternating, `rounds` times
          each, every iteration saved (burn 0, thin 1); the chain and the conditional criteria must be identical in both.
    python profiles/micro/rows_loo_time.py [micro|fit|both] [side] [keep] [rounds]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, fit  # noqa: E402
from spamtree_amd.model import SpamTreeMV, _dp  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def timed(hm, call, reps):
    for _ in range(3):
        call()
    hm.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        hm.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts))


def micro(wl, reps=30):
    n = int(wl["n"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.random.default_rng(1).standard_normal(n), wl["beta_true"], wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    hm.rows_loo_set()
    info = hm.rows_loo_info()
    loo_med, loo_min = timed(hm, hm.rows_loo_accumulate, reps)
    it = [0]

    def sim():
        it[0] += 1
        hm._check(hm.lib.st_simulate(hm.h, 1, None, None, 2021, it[0], None, None))
    sim_med, sim_min = timed(hm, sim, reps)
    loo_med2, loo_min2 = timed(hm, hm.rows_loo_accumulate, reps)      # again behind it: the order of the two does not matter
    peaks = np.zeros(3)
    hm._check(hm.lib.st_probe_peaks(0, 8 * n * 16, 5, _dp(peaks)))
    t0 = time.perf_counter()
    tot = hm.rows_loo_totals()
    totals_ms = 1e3 * (time.perf_counter() - t0)
    res = dict(n=n, routes=info["routes"], alg_bytes=info["alg_bytes"], flops=info["flops"], panel_bytes=hm.simulate_info(1)["alg_bytes"],
               accumulate_sync_ms_median=loo_med, accumulate_sync_ms_min=loo_min, accumulate_again_ms_median=loo_med2,
               simulate_nd1_sync_ms_median=sim_med, simulate_nd1_sync_ms_min=sim_min, copy_GBps=float(peaks[0]),
               fraction_of_copy_bandwidth_sync=info["alg_bytes"] / (loo_med * 1e-3) / (peaks[0] * 1e9), totals_ms=totals_ms,
               elpd_loo=tot["elpd_loo"], min_weight_ess=tot["min_weight_ess"])
    hm.close()
    return res


def run(wl, keep, **kw):
    out = fit.spamtree_mv_mcmc(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                               wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                               wl["bounds"], np.zeros(wl["n"]), wl["theta"], np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size),
                               mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False,
                               save_yhat=False, main_verbose=False, criteria=True, **kw)
    return out, 1e3 * out["mcmc_time"] / keep


def fits(wl, keep, rounds):
    run(wl, 3)                          # warm-up: code objects, allocations
    run(wl, 3, loo=True)
    base, feat = [], []
    for _ in range(rounds):
        ob, tb = run(wl, keep)
        of, tf = run(wl, keep, loo=True)
        base.append(tb)
        feat.append(tf)
        for key in ("theta_mcmc", "beta_mcmc", "tausq_mcmc"):
            assert np.array_equal(ob[key], of[key]), key
        assert np.array_equal(ob["criteria"]["lppd"], of["criteria"]["lppd"], equal_nan=True)
    lo = of["criteria"]["loo"]["totals"]
    return dict(ms_per_saved_iter_criteria=base, ms_per_saved_iter_criteria_and_loo=feat,
                added_ms_median=float(np.median(np.array(feat) - np.array(base))), spread_without_ms=float(max(base) - min(base)),
                spread_with_ms=float(max(feat) - min(feat)), waic=of["criteria"]["totals"]["observed"]["waic"], looic=lo["looic"],
                min_weight_ess=lo["min_weight_ess"], keep=keep)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    a = [int(x) for x in sys.argv[2:]]
    side, keep, rounds = (a + [1000, 30, 3][len(a):])[:3]
    _lib.load()
    wl = make_workload(side, device=0)
    res = {}
    if what in ("micro", "both"):
        res["micro"] = micro(wl)
        print("micro", json.dumps(res["micro"]), flush=True)
    if what in ("fit", "both"):
        res["fit"] = fits(wl, keep, rounds)
        print("fit", json.dumps(res["fit"]), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
