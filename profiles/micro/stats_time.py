"""Diagnostic (not part of the product): what wide X costs at config #3's tree (n = 1e6, q = 1) with p = 3, 8, 9, 16 and 64
covariates (X of the p = 3 workload with standard-normal columns appended; the tree is built once).  Per p, one JSON line:
  create_s       wall time of SpamTreeMV(...) (st_create and the first setters; p > 8 forms XtX on the device in it)
  stats_ms       one statistics reduction (k_stats + k_stats_final) from the library's HIP events around the launch
                 (st_profile_enable(1), family 4), median of 10 after 3 warm-up calls, each after an st_set_w
  stats_GBps     the bytes the kernel really reads over that time: 8 n p for X, and per slice of eight columns the row vectors
                 obs (1), mv (4), y (8), partner (8), w[partner] (8) = 29 n; slice 0 also xb and w of the row (16 n)
  copy_GBps      st_probe_peaks' stream copy (read + written bytes) on the same device, for comparison
  chain_it_s     Chain.step throughput, 30 steps after 10 of warm-up, wall time ending in a device synchronise
The share of create that is XtX: run this script under `rocprofv3 --kernel-trace --stats` in a run of its own and add up
k_stats<1, true> and the k_stats_final launches of create (p of each per handle).
    python profiles/micro/stats_time.py [p ...]        (default 3 8 9 16 64)"""
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

SIDE = int(os.environ.get("STATS_TIME_SIDE", "1000"))


def stats_bytes(n, p):
    slices = (p + 7) // 8
    return 8.0 * n * p + 29.0 * n * slices + 16.0 * n


def main(ps):
    wl = make_workload(SIDE, q=1, p=3)
    n = wl["n"]
    rng = np.random.default_rng(7)
    extra = rng.standard_normal((n, max(max(ps) - 3, 0)))
    pk = np.zeros(3)
    assert _lib.load().st_probe_peaks(0, 1 << 30, 5, _dp(pk)) == 0
    copy_gbps = float(pk[0])
    for p in ps:
        X = np.asfortranarray(np.hstack([wl["X"], extra[:, :p - 3]])) if p > 3 else np.asfortranarray(wl["X"][:, :p])
        beta = np.r_[wl["beta_true"], np.zeros(max(p - 3, 0))][:p]
        t0 = time.perf_counter()
        hm = SpamTreeMV(wl["y"], X, wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                        wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                        np.zeros(n), beta, wl["theta"], 10.0, device=0)
        hm.synchronize()
        create_s = time.perf_counter() - t0
        xty = np.zeros(p)
        hm.profile(1)
        ms = []
        for r in range(13):
            hm.set_w(rng.standard_normal(n))
            hm.synchronize()
            hm.profile_get()
            hm._check(hm.lib.st_beta_stats(hm.h, _dp(xty)))
            hm.synchronize()
            got = hm.profile_get()["stats"]
            assert got[1] == 1, got
            if r >= 3:
                ms.append(got[0])
        hm.profile(0)
        hm.close()
        stats_ms = float(np.median(ms))
        ch = fit.Chain(wl["y"], X, wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                       wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                       wl["bounds"], wl["theta"], np.zeros(p), 0.1, 0.01 * np.eye(wl["theta"].size), seed=5)
        ch.step(10)
        ch.synchronize()
        t0 = time.perf_counter()
        ch.step(30)
        ch.synchronize()
        it_s = 30.0 / (time.perf_counter() - t0)
        ch.close()
        by = stats_bytes(n, p)
        print(json.dumps(dict(n=n, p=p, slices=(p + 7) // 8, create_s=create_s, stats_ms=stats_ms, stats_ms_min=float(min(ms)),
                              stats_ms_max=float(max(ms)), stats_bytes=by, stats_GBps=by / (stats_ms * 1e-3) / 1e9,
                              copy_GBps=copy_gbps, chain_it_s=it_s)), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [3, 8, 9, 16, 64])
