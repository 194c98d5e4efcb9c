"""Diagnostic (not part of the product): cost of scoring held-out observations at the new points (stm_mcmc_scored,
predict.fit_predict(y_new=)) at config #3's tree, against the same fit_predict without y_new (stm_mcmc_points(_joint): no score step
runs, no draw is stored).  New points: the side x side grid offset by half a grid step, plain and in joint
groups of four consecutive cells; y_new: the workload's smooth field is not available off the grid, so standard normals plus the
regression -- the cost does not depend on the values.  Summaries only, nothing saved per draw; every iteration is saved (burn 0,
thin 1), so fit milliseconds per iteration = per saved iteration.  With y_new the fit also keeps the yhat and w draws on the device
for the CRPS (16 B a point and saved iteration), which is part of the added time.  The two variants alternate, `rounds` times each;
the chain and the predictive means must be identical in both.  Then the one-off cost of st_points_score_get at `crps_keep` stored
draws, with and without the CRPS, on a handle of its own.
    python profiles/micro/score_time.py [side] [keep] [grid_side] [rounds] [crps_keep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import SpamTreeMV  # noqa: E402
from spamtree_amd.predict import fit_predict, locate  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def setup(side, grid_side):
    wl = make_workload(side, device=0)
    g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    rng = np.random.default_rng(3)
    Xn = rng.standard_normal((pts.shape[0], wl["p"]))
    y = Xn @ wl["beta_true"] + 1.5 * rng.standard_normal(pts.shape[0])
    y[rng.uniform(size=y.size) < 0.1] = np.nan
    return wl, pts, Xn, y


def run(wl, pts, Xn, y, joint, keep):
    out = fit_predict(wl, pts, np.ones(pts.shape[0], dtype=np.int64), Xn, return_draws=False, joint=joint, y_new=y, mcmc_keep=keep,
                      mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False, save_yhat=False)
    return out, 1e3 * out["mcmc_time"] / keep


def get_time(wl, pts, Xn, y, crps_keep):
    """Wall time of st_points_score_get over crps_keep stored draws (one state: the values do not matter), ms."""
    mv = np.ones(pts.shape[0], dtype=np.int64)
    p = int(wl["p"])
    hm = SpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"], wl["res_is_ref"],
                    wl["parents"], wl["children"], False, wl["block_names"], wl["block_groups"], wl["indexing"],
                    np.zeros(int(wl["n"])), np.zeros(p), wl["theta"], 10.0, device=0)
    assert hm.get_loglik_comps_w(0)
    hm.set_points(pts, mv, locate(wl["topo"], pts, mv, device=0), Xn)
    hm.set_scores(y)
    hm._check(hm.lib.st_points_summary_reserve(hm.h, crps_keep))
    for s in range(crps_keep):
        hm._check(hm.lib.st_points_accumulate(hm.h, 11, s, None, None, None, None))
    hm.synchronize()
    res = {}
    for name, crps in (("get_without_crps_ms", False), ("get_with_crps_ms", True)):
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            sc = hm.scores(crps=crps)
            ts.append(1e3 * (time.perf_counter() - t0))
        res[name] = ts[1:]                                  # the first call loads the code object
    res["mean_crps"] = sc["totals"]["crps"]
    hm.close()
    return res


def main():
    a = [int(x) for x in sys.argv[1:]]
    side, keep, grid_side, rounds, crps_keep = (a + [1000, 50, 1000, 3, 1000][len(a):])[:5]
    wl, pts, Xn, y = setup(side, grid_side)
    n = pts.shape[0]
    print(f"n = {wl['n']}, {n} new points, {int(np.sum(~np.isnan(y)))} scored, keep {keep}", flush=True)
    res = dict(new_points=n, keep=keep)
    for tag, joint in (("plain", None), ("groups_of_4", np.arange(n) // 4)):
        run(wl, pts, Xn, None, joint, 3)        # warm-up: code objects, allocations
        run(wl, pts, Xn, y, joint, 3)
        base, feat = [], []
        for _ in range(rounds):
            ob, tb = run(wl, pts, Xn, None, joint, keep)
            of, tf = run(wl, pts, Xn, y, joint, keep)
            base.append(tb)
            feat.append(tf)
            assert np.array_equal(ob["theta_mcmc"], of["theta_mcmc"]) and np.array_equal(ob["new"]["mean"], of["new"]["mean"])
            assert np.array_equal(ob["beta_mcmc"], of["beta_mcmc"]) and np.array_equal(ob["tausq_mcmc"], of["tausq_mcmc"])
        sc = of["new"]["scores"]
        res[tag] = dict(ms_per_saved_iter_without=base, ms_per_saved_iter_with=feat,
                        added_ms_median=float(np.median(np.array(feat) - np.array(base))),
                        spread_without_ms=float(max(base) - min(base)), spread_with_ms=float(max(feat) - min(feat)),
                        mean_lpd=sc["totals"]["lpd"], mean_crps=sc["totals"]["crps"], n_degenerate=sc["n_degenerate"],
                        accepted=len({tuple(c) for c in of["theta_mcmc"].T}))
        print(tag, json.dumps(res[tag]), flush=True)
    if crps_keep > 0:
        res["score_get"] = dict(get_time(wl, pts, Xn, y, crps_keep), stored_draws=crps_keep)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
