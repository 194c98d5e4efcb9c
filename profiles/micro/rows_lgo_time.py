"""Diagnostic (not part of the product): cost of the leave-group-out criteria (st_rows_loo_groups_*) at config #3's tree
(n = 1e6, q = 1, every row observed) with 2 x 2-cell labels (250 000 groups of four).
On one handle, device-synchronised medians of st_rows_loo_accumulate without groups, with groups, and without again (st_rows_loo_set
anew between them), `rounds` times alternating; st_rows_loo_info's bytes with and without; the copy bandwidth st_probe_peaks measures
on the same box; then, with a store of `draws` draws, the group PSIS (st_rows_loo_groups_psis) once.
    python profiles/micro/rows_lgo_time.py [side] [rounds] [draws]
Against another build of the library (the parent commit's tree, built, at OTHER): `rounds` times alternating, each leg a fresh child
process that imports spamtree_amd from the tree it is given and times st_rows_loo_accumulate on a handle of its own:
OTHER without groups, this tree without groups, this tree with groups.
    python profiles/micro/rows_lgo_time.py against OTHER [side] [rounds]
One leg alone (what `against` starts; under `rocprofv3 --kernel-trace --stats -- python ... leg . with` the trace has k_lgo_groups'
and k_loo_block's own times):
    python profiles/micro/rows_lgo_time.py leg TREE with|without [side]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "leg" else HERE   # a leg imports the tree it is given
sys.path.insert(0, ROOT)
from spamtree_amd import _lib  # noqa: E402
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


def cell_labels(coords, k):
    ix = np.searchsorted(np.unique(coords[:, 0]), coords[:, 0]) // k
    iy = np.searchsorted(np.unique(coords[:, 1]), coords[:, 1]) // k
    return (ix * (iy.max() + 1) + iy).astype(np.int64)


def make_handle(side):
    wl = make_workload(side, device=0)
    n = int(wl["n"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.random.default_rng(1).standard_normal(n), wl["beta_true"], wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    return wl, hm


def leg(groups, side):
    """One handle, st_rows_loo_accumulate timed twice (30 calls each) with or without groups; one JSON line."""
    _lib.load()
    wl, hm = make_handle(side)
    hm.rows_loo_set()
    if groups:
        hm.rows_loo_groups_set(cell_labels(np.asarray(wl["coords"]), 2))
    a, b = timed(hm, hm.rows_loo_accumulate, 30), timed(hm, hm.rows_loo_accumulate, 30)
    hm.close()
    print("leg", json.dumps(dict(tree=ROOT, groups=groups, median_ms=[a[0], b[0]], min_ms=[a[1], b[1]])), flush=True)


def against(other, side, rounds):
    """The alternating rounds; every leg in a child process of its own, one after another (this process never opens the device)."""
    legs = [("other_without", other, "without"), ("this_without", HERE, "without"), ("this_with_groups", HERE, "with")]
    res = {k: [] for k, _, _ in legs}
    for _ in range(rounds):
        for key, tree, mode in legs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "leg", tree, mode, str(side)], capture_output=True, text=True,
                                 timeout=600, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("leg ")][-1]
            res[key].append(json.loads(line[4:])["median_ms"])
            print(key, line, flush=True)
    flat = {k: [x for pair in v for x in pair] for k, v in res.items()}
    res.update(side=side, rounds=rounds, median={k: float(np.median(v)) for k, v in flat.items()},
               spread={k: float(max(v) - min(v)) for k, v in flat.items()})
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "leg":
        return leg(sys.argv[3] == "with", int(sys.argv[4]) if len(sys.argv) > 4 else 1000)
    if len(sys.argv) > 1 and sys.argv[1] == "against":
        a = [int(x) for x in sys.argv[3:]]
        return against(os.path.abspath(sys.argv[2]), *(a + [1000, 3][len(a):])[:2])
    a = [int(x) for x in sys.argv[1:]]
    side, rounds, draws = (a + [1000, 3, 1000][len(a):])[:3]
    _lib.load()
    wl = make_workload(side, device=0)
    n = int(wl["n"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.random.default_rng(1).standard_normal(n), wl["beta_true"], wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    labels = cell_labels(np.asarray(wl["coords"]), 2)
    without, with_groups, set_s = [], [], []
    for _ in range(rounds):
        hm.rows_loo_set()
        base = hm.rows_loo_info()
        without.append(timed(hm, hm.rows_loo_accumulate, 30)[0])
        hm.rows_loo_set()
        t0 = time.perf_counter()
        hm.rows_loo_groups_set(labels)
        set_s.append(time.perf_counter() - t0)
        info = hm.rows_loo_info()
        with_groups.append(timed(hm, hm.rows_loo_accumulate, 30)[0])
    ix = hm.rows_loo_groups_index()
    tot = hm.rows_loo_groups_totals()
    peaks = np.zeros(3)
    hm._check(hm.lib.st_probe_peaks(0, 8 * n * 16, 5, _dp(peaks)))
    res = dict(n=n, n_groups=ix["n_groups"], n_members=ix["n_members"], n_pairs=ix["n_pairs"], accumulate_without_ms=without,
               accumulate_with_groups_ms=with_groups, added_ms_median=float(np.median(np.array(with_groups) - np.array(without))),
               alg_bytes_without=base["alg_bytes"], alg_bytes_with=info["alg_bytes"], copy_GBps=float(peaks[0]),
               predicted_added_ms=(info["alg_bytes"] - base["alg_bytes"]) / (peaks[0] * 1e9) * 1e3, groups_set_s=set_s,
               elpd_lgo=tot["elpd_lgo"], min_weight_ess=tot["min_weight_ess"])
    print("accumulate", json.dumps(res), flush=True)
    if draws > 0:
        hm.rows_loo_set()
        hm.rows_loo_reserve(draws)
        hm.rows_loo_groups_set(labels)
        rng = np.random.default_rng(2)
        for _ in range(draws):
            hm.set_w(rng.standard_normal(n))
            hm.rows_loo_accumulate()
        hm.synchronize()
        t0 = time.perf_counter()
        ps = hm.rows_loo_groups_psis()
        res.update(psis_draws=draws, group_psis_ms=1e3 * (time.perf_counter() - t0), max_khat=float(np.nanmax(ps["khat"])))
    hm.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
