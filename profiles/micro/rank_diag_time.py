"""Diagnostic (not part of the product): cost of the rank-normalised diagnostics of the stored draws
(st_summary_rank_diagnostics, k_series_rank) beside st_summary_diagnostics (k_series_diag) and st_summary_quantile (k_qtile) on
the same store, in one run.  Config #3's tree (side x side rows); the store is filled by the chain itself: `keep` iterations of
stm_step, each followed by st_summary_accumulate, so the rows' autocorrelation is the sampler's own.
  device   st_profile_get's event time around each launch (family `reduce`): k_series_rank with the bulk and folded outputs alone
           (rhat_rank, ess_bulk: two sorts, two rank passes, the moments and the lag passes) and with 8 probabilities and 8
           thresholds on top (every output; 18 indicator series with the two tails); k_series_diag with the default lag cap;
           k_qtile for one q
  wall     the same calls as a user makes them, host-synchronous, with the copy of the requested outputs
Under `rocprofv3 --kernel-trace --stats -- python ...` the trace has the kernels' own times.
    python profiles/micro/rank_diag_time.py [side] [keep] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, diagnostics, fit  # noqa: E402
from spamtree_amd.model import _dp, rank_buffers, rank_spec  # noqa: E402
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
    q = int(wl["q"]) if "q" in wl else 1
    probs = (0.025, 0.05, 0.25, 0.5, 0.75, 0.9, 0.95, 0.975)
    thresholds = [float(v) for v in np.linspace(-1.5, 1.5, 8)]
    spec0, keep0, _, _ = rank_spec((), (), None, 0, q)
    spec8, keep8, n_prob, n_thr = rank_spec(probs, thresholds, [1, -1] * 4, 0, q)
    d0, _ = rank_buffers(n, 0, 0)
    bulk_fold = _lib.StRankOut(rhat_rank=_dp(d0["rhat_rank"]), ess_bulk=_dp(d0["ess_bulk"]))
    d8, every = rank_buffers(n, n_prob, n_thr)
    wq, ess = np.zeros(n), np.zeros(n)
    only_ess = _lib.StSeriesDiag(_dp(ess), None, None, None, None)
    t = dict(rank_bulk_fold=[], rank_all=[], diag=[], qtile=[])
    w = dict(rank_bulk_fold=[], rank_all=[], diag=[], qtile=[])

    def timed(key, call):
        ch.profile(1)
        ch.profile_get()
        t0 = time.perf_counter()
        assert call() == 0
        w[key].append(1e3 * (time.perf_counter() - t0))
        t[key].append(ch.profile_get()["reduce"][0])
        ch.profile(0)

    for _ in range(reps):
        timed("rank_bulk_fold", lambda: lib.st_summary_rank_diagnostics(h, C.byref(spec0), C.byref(bulk_fold), None))
        timed("rank_all", lambda: lib.st_summary_rank_diagnostics(h, C.byref(spec8), C.byref(every), None))
        timed("diag", lambda: lib.st_summary_diagnostics(h, 0, C.byref(only_ess), None))
        t0 = time.perf_counter()
        assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == 0
        w["qtile"].append(1e3 * (time.perf_counter() - t0))
    del keep0, keep8
    bw = lambda ms: store_bytes / (ms * 1e-3) / (peaks[0] * 1e9) if ms > 0 else None   # noqa: E731
    res.update(device_ms=t, wall_ms=w, rank_bulk_fold_fraction_of_copy_bandwidth=bw(min(t["rank_bulk_fold"])),
               rank_all_fraction_of_copy_bandwidth=bw(min(t["rank_all"])), diag_fraction_of_copy_bandwidth=bw(min(t["diag"])),
               mean_lags_bulk=float(np.mean(d8["lags_bulk"])), max_lags_bulk=int(np.max(d8["lags_bulk"])),
               summary=diagnostics.summarise_rank(d8))
    print(json.dumps(res), flush=True)
    ch.close()


if __name__ == "__main__":
    main()
