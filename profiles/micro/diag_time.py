"""Diagnostic (not part of the product): cost of the convergence diagnostics of the stored draws (st_summary_diagnostics,
k_series_diag) beside st_summary_quantile for one q on the same store -- both read the store once.  Config #3's tree (side x
side rows); the store is filled by the chain itself: `keep` iterations of stm_step, each followed by st_summary_accumulate, so
the rows' autocorrelation is the sampler's own.
  wall     the calls as a user makes them, host-synchronous: launch, kernel, the copy of the requested outputs and their
           permutation to model row order (quantile: n doubles; diagnostics: `ess` alone, then all five)
  device   st_profile_get's event time around the diagnostics launch (family `reduce`), with the default lag cap and with
           max_lag = 1 (one pass over the lags: what staging and the moments cost by themselves)
Under `rocprofv3 --kernel-trace --stats -- python ... ` the trace has both kernels' own times (k_qtile, k_series_diag).
    python profiles/micro/diag_time.py [side] [keep] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, diagnostics, fit  # noqa: E402
from spamtree_amd.model import _dp, series_diag_buffers  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    side, keep, reps = (a + [1000, 1000, 3][len(a):])[:3]
    lib = _lib.load()
    wl = make_workload(side, device=0)
    n = int(wl["n"])
    ch = fit.Chain(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"], wl["parents"],
                   wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"], wl["bounds"], wl["theta"],
                   np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size), seed=11, adapting=True, device=0)
    h = ch.h
    assert lib.st_summary_reserve(h, keep) == 0
    t0 = time.perf_counter()
    for it in range(keep):
        ch.step(1)
        assert lib.st_summary_accumulate(h, 11, it) == 0
    ch.synchronize()
    fill_s = time.perf_counter() - t0
    peaks = np.zeros(3)
    assert lib.st_probe_peaks(0, 1 << 30, 5, _dp(peaks)) == 0
    store_bytes = 8.0 * keep * n
    res = dict(n=n, keep=keep, store_GB_per_quantity=store_bytes / 1e9, fill_s=fill_s, copy_GBps=float(peaks[0]))
    wq = np.zeros(n)
    d, s = series_diag_buffers(n)
    only_ess = _lib.StSeriesDiag(_dp(d["ess"]), None, None, None, None)
    tq, te, ta, dev, dev1 = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == 0
        tq.append(1e3 * (time.perf_counter() - t0))
        ch.profile(1)
        ch.profile_get()
        t0 = time.perf_counter()
        assert lib.st_summary_diagnostics(h, 0, C.byref(only_ess), None) == 0
        te.append(1e3 * (time.perf_counter() - t0))
        dev.append(ch.profile_get()["reduce"][0])
        assert lib.st_summary_diagnostics(h, 1, C.byref(only_ess), None) == 0      # one pair of lags: staging and moments alone
        dev1.append(ch.profile_get()["reduce"][0])
        ch.profile(0)
        t0 = time.perf_counter()
        assert lib.st_summary_diagnostics(h, 0, C.byref(s), None) == 0
        ta.append(1e3 * (time.perf_counter() - t0))
    d["truncated"] = diagnostics.truncated(d["lags"], keep)
    res.update(quantile_w_wall_ms=tq, diagnostics_w_ess_only_wall_ms=te, diagnostics_w_all_wall_ms=ta, diagnostics_w_device_ms=dev, diagnostics_w_max_lag_1_device_ms=dev1,
               diagnostics_fraction_of_copy_bandwidth=store_bytes / (min(dev) * 1e-3) / (peaks[0] * 1e9) if min(dev) > 0 else None,
               mean_lags=float(np.mean(d["lags"])), max_lags=int(np.max(d["lags"])), summary=diagnostics.summarise(d))
    print(json.dumps(res), flush=True)
    ch.close()


if __name__ == "__main__":
    main()
