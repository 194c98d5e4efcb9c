"""Diagnostic (not part of the product): cost of the exceedance / excursion / band passes over the stored draws
(st_summary_excursions: k_store_colstats, k_store_drawreduce and the finish) beside st_summary_diagnostics with max_lag = 1 and
st_summary_quantile for one q on the same store -- each reads the store once.  A grid workload (config #3: side 1000, q = 1;
config #4's shape: side 577, q = 3); the store is filled by the chain itself: `keep` iterations of stm_step, each followed by
st_summary_accumulate.
  wall     the call as a user makes it, host-synchronous, for w alone with every output asked for: the small uploads, the
           launches, the copies of the outputs and their permutation to model row order
  device   st_profile_get's event time around the launches of one call (family `reduce`): both passes and the finish together
  bytes    from the shapes: pass 1 reads the store once (8 K n) and writes 4 T n + 16 n; pass 2 reads the store once and, per
           chunk of draws, the side data (4 T + 17 bytes per series with the band)
Three requests: T = 1 without the band, T = 1 with it, T = 8 (mixed sides) with it.  The kernels' own times -- one row per
instantiation: k_store_colstats<T', band>, k_store_drawreduce<T', band, S> -- are in the trace of
    rocprofv3 --kernel-trace --stats -- python profiles/micro/excursions_time.py [side] [keep] [reps] [q]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, fit  # noqa: E402
from spamtree_amd.model import _dp, excursion_buffers, excursion_spec, series_diag_buffers  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    side, keep, reps, q = (a + [1000, 1000, 3, 1][len(a):])[:4]
    lib = _lib.load()
    wl = make_workload(side, q=q, device=0)
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
    res = dict(n=n, q=q, keep=keep, store_GB_per_quantity=store_bytes / 1e9, fill_s=fill_s, copy_GBps=float(peaks[0]))
    sides8 = np.array([1, -1, 1, -1, 1, -1, 1, -1], dtype=np.int32)
    thr8 = np.repeat(np.linspace(-1.5, 1.5, 8)[:, None], q, axis=1)
    requests = dict(T1=(thr8[3:4].copy(), sides8[:1].copy(), False), T1_band=(thr8[3:4].copy(), sides8[:1].copy(), True),
                    T8_band=(np.ascontiguousarray(thr8), sides8, True))
    for name, (thr, sd, band) in requests.items():
        spec, keepalive = excursion_spec(np.ascontiguousarray(thr), sd, None, band)
        d, o = excursion_buffers(n, thr.shape[0], q, keep, band)
        wall, dev = [], []
        for _ in range(reps):
            ch.profile(1)
            ch.profile_get()
            t0 = time.perf_counter()
            assert lib.st_summary_excursions(h, C.byref(spec), C.byref(o), None) == 0, lib.st_last_error(h)
            wall.append(1e3 * (time.perf_counter() - t0))
            dev.append(ch.profile_get()["reduce"][0])
            ch.profile(0)
        T = thr.shape[0]
        res[name] = dict(wall_ms=wall, device_ms=dev, store_reads=2,
                         fraction_of_copy_bandwidth_both_passes=2 * store_bytes / (min(dev) * 1e-3) / (peaks[0] * 1e9) if min(dev) > 0 else None,
                         joint_all=d["joint_all"].tolist(), max_prob=float(d["prob"].max()), max_excur=float(np.nanmax(d["excur"])),
                         pass1_bytes=store_bytes + (4.0 * T + (16.0 if band else 0.0)) * n)
        del keepalive
    # beside them, on the same store: the diagnostics with one pair of lags (staging and moments alone) and one quantile
    wq = np.zeros(n)
    dd, s = series_diag_buffers(n)
    only_ess = _lib.StSeriesDiag(_dp(dd["ess"]), None, None, None, None)
    tq, dev1 = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert lib.st_summary_quantile(h, 0.5, _dp(wq), None) == 0
        tq.append(1e3 * (time.perf_counter() - t0))
        ch.profile(1)
        ch.profile_get()
        assert lib.st_summary_diagnostics(h, 1, C.byref(only_ess), None) == 0
        dev1.append(ch.profile_get()["reduce"][0])
        ch.profile(0)
    res.update(quantile_w_wall_ms=tq, diagnostics_w_max_lag_1_device_ms=dev1)
    print(json.dumps(res), flush=True)
    ch.close()


if __name__ == "__main__":
    main()
