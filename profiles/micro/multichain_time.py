"""Diagnostic (not part of the product): cost of the multi-chain diagnostics of the stored draws (st_summary_chain_diagnostics,
st_summary_chain_rank_diagnostics: k_series_diag<true>, k_series_rank<true>) beside the single-chain calls on the SAME store, in
the same run, alternating -- the single-chain call is the baseline, never an earlier run.  diag_time.py's shape: config #3's
tree (side x side rows), the store filled by the chain itself (`keep` iterations of stm_step, each followed by
st_summary_accumulate); the multi-chain calls read its K = keep draws as M chains of keep / M.
  wall     the calls as a user makes them, host-synchronous, all outputs of w (plain: the five; rank: rhat_rank, rhat_bulk,
           rhat_fold, ess_bulk, ess_tail, lags_bulk)
  device   st_profile_get's event time around the launch (family `reduce`)
  *_lag8   the same four calls with max_lag = 8 (two lag passes at the most in either): the cost of the per-chain moments by
           themselves, apart from how many lags the definition makes a series walk (mean_lags has both)
Every figure is a list over the repetitions; `least` holds the least of each and the ratios multi / single, `spread` the largest
relative distance between two repetitions of a single-chain call.
    python profiles/micro/multichain_time.py [side] [keep] [chains] [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd import _lib, fit  # noqa: E402
from spamtree_amd.model import rank_buffers, rank_spec, series_diag_buffers  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    side, keep, M, reps = (a + [700, 500, 4, 3][len(a):])[:4]
    assert keep % M == 0
    lib = _lib.load()
    wl = make_workload(side, device=0)
    n = int(wl["n"])
    ch = fit.Chain(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"], wl["parents"],
                   wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"], wl["bounds"], wl["theta"],
                   np.zeros(wl["p"]), 0.1, 0.01 * np.eye(wl["theta"].size), seed=11, adapting=True, device=0)
    h = ch.h
    assert lib.st_summary_reserve(h, keep) == 0
    for it in range(keep):
        ch.step(1)
        assert lib.st_summary_accumulate(h, 11, it) == 0
    ch.synchronize()
    d, s = series_diag_buffers(n)
    spec, hold, n_prob, n_thr = rank_spec((), (), None, 0, 1)
    dr, o = rank_buffers(n, n_prob, n_thr)
    spec8, hold8, _, _ = rank_spec((), (), None, 8, 1)
    # *_lag8: max_lag = 8, at most two lag passes in either call -- what the per-chain moments cost by themselves, apart from how
    # many lags the definition makes a series walk
    calls = dict(plain_single=lambda: lib.st_summary_diagnostics(h, 0, C.byref(s), None),
                 plain_multi=lambda: lib.st_summary_chain_diagnostics(h, M, 0, C.byref(s), None),
                 rank_single=lambda: lib.st_summary_rank_diagnostics(h, C.byref(spec), C.byref(o), None),
                 rank_multi=lambda: lib.st_summary_chain_rank_diagnostics(h, M, C.byref(spec), C.byref(o), None),
                 plain_single_lag8=lambda: lib.st_summary_diagnostics(h, 8, C.byref(s), None),
                 plain_multi_lag8=lambda: lib.st_summary_chain_diagnostics(h, M, 8, C.byref(s), None),
                 rank_single_lag8=lambda: lib.st_summary_rank_diagnostics(h, C.byref(spec8), C.byref(o), None),
                 rank_multi_lag8=lambda: lib.st_summary_chain_rank_diagnostics(h, M, C.byref(spec8), C.byref(o), None))
    wall, dev, lags = {k: [] for k in calls}, {k: [] for k in calls}, {}
    for _ in range(reps):
        for name, call in calls.items():   # single, multi, single, multi: alternating
            ch.profile(1)
            ch.profile_get()
            t0 = time.perf_counter()
            assert call() == 0
            wall[name].append(1e3 * (time.perf_counter() - t0))
            dev[name].append(ch.profile_get()["reduce"][0])
            ch.profile(0)
            lags[name] = float(np.mean(d["lags"] if name.startswith("plain") else dr["lags_bulk"]))
    least = {f"{k}_{what}_ms": min(v[k]) for what, v in (("wall", wall), ("device", dev)) for k in calls}
    for fam in ("plain", "rank"):
        for what in ("wall", "device"):
            for cap in ("", "_lag8"):
                least[f"{fam}{cap}_{what}_ratio"] = least[f"{fam}_multi{cap}_{what}_ms"] / least[f"{fam}_single{cap}_{what}_ms"]
    spread = {f"{k}_{what}": (max(v[k]) - min(v[k])) / min(v[k]) for what, v in (("wall", wall), ("device", dev)) for k in calls if "single" in k}
    print(json.dumps(dict(n=n, keep=keep, chains=M, draws_per_chain=keep // M, wall_ms=wall, device_ms=dev, mean_lags=lags, least=least,
                          spread=spread)), flush=True)
    ch.close()


if __name__ == "__main__":
    main()
