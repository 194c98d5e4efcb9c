"""Diagnostic (not part of the product): cost of the criteria over the fit's own rows (st_rows_score_*, stm_mcmc_criteria) at
config #3's tree with 10 % of the rows NA and held out.  The held-out values are the regression plus standard normals: the cost
does not depend on them.
  micro   on a handle of its own: the device-synchronised median of st_rows_score_accumulate against the copy bandwidth
          st_probe_peaks measures on the same box and st_rows_score_info's bytes; st_rows_score_totals once; st_rows_score_get with
          the CRPS over `crps_keep` stored draws once.  Under `rocprofv3 --kernel-trace --stats -- python ... micro` the trace has
          the kernels' own times.
  fit     fit.spamtree_mv_mcmc(save_w=False, save_yhat=False) with and without y_holdout, alternating, `rounds` times each, every
          iteration saved (burn 0, thin 1); the chain must be identical in both.  holdout_crps=False: the accumulate step alone.
    python profiles/micro/rows_score_time.py [micro|fit|both] [side] [keep] [rounds] [crps_keep]"""
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


def setup(side):
    wl = make_workload(side, missing=(0.1,), device=0)
    rng = np.random.default_rng(3)
    na = np.isnan(wl["y"])
    hold = np.where(na, wl["X"] @ wl["beta_true"] + 1.5 * rng.standard_normal(wl["n"]), np.nan)
    return wl, hold


def micro(wl, hold, crps_keep, reps=30):
    p, n = int(wl["p"]), int(wl["n"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.random.default_rng(1).standard_normal(n), wl["beta_true"], wl["theta"], 10.0, device=0)
    hm.rows_score_set(hold, y=wl["y"])
    by = hm.rows_score_info()["alg_bytes"]
    for _ in range(3):
        hm.rows_score_accumulate()
    hm.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hm.rows_score_accumulate()
        hm.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    peaks = np.zeros(3)
    hm._check(hm.lib.st_probe_peaks(0, 8 * n * 16, 5, _dp(peaks)))
    med = float(np.median(ts))
    res = dict(n=n, targeted=int(np.sum(np.isfinite(wl["y"]) | np.isfinite(hold))), held_out=int(np.sum(np.isfinite(hold))),
               alg_bytes=by, accumulate_sync_ms_median=med, accumulate_sync_ms_min=float(min(ts)), copy_GBps=float(peaks[0]),
               fraction_of_copy_bandwidth_sync=by / (med * 1e-3) / (peaks[0] * 1e9))
    tt = []
    for _ in range(3):
        t0 = time.perf_counter()
        tot = hm.rows_score_totals()
        tt.append(1e3 * (time.perf_counter() - t0))
    res.update(totals_ms=tt, waic=tot["observed"]["waic"], dic=tot["observed"]["dic"])
    if crps_keep > 0:
        hm._check(hm.lib.st_summary_reset(hm.h))
        hm._check(hm.lib.st_summary_reserve(hm.h, crps_keep))
        for s in range(crps_keep):
            hm._check(hm.lib.st_summary_accumulate(hm.h, 11, s))
        hm.synchronize()
        tg = []
        for _ in range(3):
            t0 = time.perf_counter()
            g = hm.rows_score_get(crps=True)
            tg.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        hm.rows_score_get(crps=False)
        res.update(get_with_crps_ms=tg, get_without_crps_ms=1e3 * (time.perf_counter() - t0), stored_draws=crps_keep,
                   mean_crps=float(np.nanmean(g["crps"])))
    hm.close()
    return res


def run(wl, keep, **kw):
    out = fit.spamtree_mv_mcmc(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                               wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                               wl["bounds"], np.zeros(wl["n"]), wl["theta"], np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size),
                               mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False,
                               save_yhat=False, main_verbose=False, **kw)
    return out, 1e3 * out["mcmc_time"] / keep


def fits(wl, hold, keep, rounds):
    res = {}
    for tag, kw in (("criteria_and_crps", dict(y_holdout=hold)), ("criteria_only", dict(y_holdout=hold, holdout_crps=False))):
        run(wl, 3)                          # warm-up: code objects, allocations
        run(wl, 3, **kw)
        base, feat = [], []
        for _ in range(rounds):
            ob, tb = run(wl, keep)
            of, tf = run(wl, keep, **kw)
            base.append(tb)
            feat.append(tf)
            for key in ("theta_mcmc", "beta_mcmc", "tausq_mcmc"):
                assert np.array_equal(ob[key], of[key]), key
        o = of["criteria"]["totals"]
        res[tag] = dict(ms_per_saved_iter_without=base, ms_per_saved_iter_with=feat,
                        added_ms_median=float(np.median(np.array(feat) - np.array(base))),
                        spread_without_ms=float(max(base) - min(base)), spread_with_ms=float(max(feat) - min(feat)),
                        waic=o["observed"]["waic"], dic=o["observed"]["dic"], held_rmse=o["held_out"]["rmse"],
                        held_crps=o["held_out"]["crps"])
        print(tag, json.dumps(res[tag]), flush=True)
    return res


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    a = [int(x) for x in sys.argv[2:]]
    side, keep, rounds, crps_keep = (a + [1000, 50, 3, 100][len(a):])[:4]
    _lib.load()
    wl, hold = setup(side)
    print(f"n = {wl['n']}, {int(np.sum(np.isfinite(hold)))} rows NA and held out", flush=True)
    res = {}
    if what in ("micro", "both"):
        res["micro"] = micro(wl, hold, crps_keep)
        print("micro", json.dumps(res["micro"]), flush=True)
    if what in ("fit", "both"):
        res["fit"] = fits(wl, hold, keep, rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
