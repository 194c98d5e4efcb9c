"""Diagnostic (not part of the product): cost of the Pareto smoothing of the leave-one-out weights (st_rows_loo_reserve,
st_rows_loo_psis: k_loo_psis and k_psis_finish) at config #3's tree (side x side rows, q = 1, every row observed).
  micro   on a chain of its own: `keep` iterations of stm_step, each followed by st_rows_loo_accumulate (into a store of `keep`
          draws) and st_summary_accumulate (into a store of the same size), so both stores hold the sampler's own draws.  Then the
          device-synchronised median of repeated calls of st_rows_loo_psis (the first call of each round alone runs the kernels: the
          outputs are kept per number of accumulated draws, so the state is re-armed by one more accumulate into a spare column),
          beside k_series_rank (rhat_rank and ess_bulk alone) and one st_summary_quantile on the store of the same size in the same
          run, and the copy bandwidth st_probe_peaks reports there.
  fit     fit.spamtree_mv_mcmc(loo=True, save_w=False, save_yhat=False) with and without psis=True, alternating, `rounds` times each,
          every iteration saved; the chain and the raw leave-one-out outputs must be identical in both.
    python profiles/micro/psis_time.py [micro|fit|both] [side] [keep] [rounds]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, fit  # noqa: E402
from spamtree_amd.model import _dp, rank_buffers, rank_spec  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def micro(wl, keep, reps=5):
    lib = _lib.load()
    n = int(wl["n"])
    ch = fit.Chain(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"], wl["parents"],
                   wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"], wl["bounds"], wl["theta"],
                   np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size), seed=11, adapting=True, device=0)
    h = ch.h
    spare = reps + 1
    assert lib.st_summary_reserve(h, keep) == 0
    assert lib.st_rows_loo_set(h) == 0 and lib.st_rows_loo_reserve(h, keep + spare) == 0
    t0 = time.perf_counter()
    for it in range(keep):
        ch.step(1)
        assert lib.st_rows_loo_accumulate(h) == 0
        assert lib.st_summary_accumulate(h, 11, it) == 0
    ch.synchronize()
    fill_s = time.perf_counter() - t0
    peaks = np.zeros(3)
    assert lib.st_probe_peaks(0, 1 << 30, 5, _dp(peaks)) == 0
    kh = np.zeros(n)
    out = _lib.StPsisOut(khat=_dp(kh))
    tot = np.zeros((len(_lib.ST_ROWS_PSIS), 1), order="F")
    spec0, keep0, _, _ = rank_spec((), (), None, 0, 1)
    d0, _ = rank_buffers(n, 0, 0)
    bulk_fold = _lib.StRankOut(rhat_rank=_dp(d0["rhat_rank"]), ess_bulk=_dp(d0["ess_bulk"]))
    wq = np.zeros(n)
    t = dict(psis=[], psis_again=[], rank_bulk_fold=[], qtile=[])

    def timed(key, call):
        ch.synchronize()
        t0 = time.perf_counter()
        assert call() == 0
        ch.synchronize()
        t[key].append(1e3 * (time.perf_counter() - t0))

    for r in range(reps):
        timed("psis", lambda: lib.st_rows_loo_psis(h, C.byref(out)))           # the kernels and the copy of khat
        timed("psis_again", lambda: lib.st_rows_loo_psis(h, C.byref(out)))     # the copy alone
        timed("rank_bulk_fold", lambda: lib.st_summary_rank_diagnostics(h, C.byref(spec0), C.byref(bulk_fold), None))
        timed("qtile", lambda: lib.st_summary_quantile(h, 0.5, _dp(wq), None))
        assert lib.st_rows_loo_accumulate(h) == 0                              # K grows by one: the next round runs the kernels again
    assert lib.st_rows_loo_psis_totals(h, _dp(tot), None) == 0
    del keep0
    info_R, info_Kpad, info_lds, info_bytes = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
    assert lib.st_psis_info(h, n, keep, 2, C.byref(info_R), C.byref(info_Kpad), C.byref(info_lds), C.byref(info_bytes)) == 0
    kernel_ms = float(np.median(np.array(t["psis"]) - np.array(t["psis_again"])))
    res = dict(n=n, keep=keep, store_GB=24.0 * keep * n / 1e9, fill_s=fill_s, copy_GBps=float(peaks[0]), sync_ms=t,
               psis_kernels_ms_median=kernel_ms, R=int(info_R.value), Kpad=int(info_Kpad.value), lds_bytes=int(info_lds.value),
               alg_bytes=float(info_bytes.value),
               fraction_of_copy_bandwidth=float(info_bytes.value) / (kernel_ms * 1e-3) / (peaks[0] * 1e9) if kernel_ms > 0 else None,
               max_khat=float(tot[6, 0]), n_khat_bad=int(tot[7, 0]), n_khat_above=int(tot[8, 0]), elpd_psis=float(tot[1, 0]))
    ch.close()
    return res


def run(wl, keep, **kw):
    out = fit.spamtree_mv_mcmc(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                               wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                               wl["bounds"], np.zeros(wl["n"]), wl["theta"], np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size),
                               mcmc_keep=keep, mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False,
                               save_yhat=False, main_verbose=False, loo=True, **kw)
    return out, 1e3 * out["mcmc_time"] / keep


def fits(wl, keep, rounds):
    run(wl, 3)                          # warm-up: code objects, allocations
    run(wl, 3, psis=True)
    base, feat = [], []
    for _ in range(rounds):
        ob, tb = run(wl, keep)
        of, tf = run(wl, keep, psis=True)
        base.append(tb)
        feat.append(tf)
        for key in ("theta_mcmc", "beta_mcmc", "tausq_mcmc"):
            assert np.array_equal(ob[key], of[key]), key
        assert np.array_equal(ob["criteria"]["loo"]["elpd_loo"], of["criteria"]["loo"]["elpd_loo"], equal_nan=True)
    ps = of["criteria"]["loo"]["psis"]["totals"]
    return dict(ms_per_saved_iter_loo=base, ms_per_saved_iter_loo_with_store=feat,
                added_ms_median=float(np.median(np.array(feat) - np.array(base))), spread_without_ms=float(max(base) - min(base)),
                spread_with_ms=float(max(feat) - min(feat)), elpd_loo=of["criteria"]["loo"]["totals"]["elpd_loo"],
                elpd_psis=ps["elpd_psis"], se=ps["se"], max_khat=ps["max_khat"], n_khat_bad=ps["n_khat_bad"], keep=keep)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    a = [int(x) for x in sys.argv[2:]]
    side, keep, rounds = (a + [1000, 1000, 3][len(a):])[:3]
    _lib.load()
    wl = make_workload(side, device=0)
    res = {}
    if what in ("micro", "both"):
        res["micro"] = micro(wl, keep)
        print("micro", json.dumps(res["micro"]), flush=True)
    if what in ("fit", "both"):
        res["fit"] = fits(wl, min(keep, 30) if what == "both" else keep, rounds)
        print("fit", json.dumps(res["fit"]), flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
