"""Diagnostic (not part of the product): cost of linear functionals of the new-point predictions (stm_mcmc_functionals,
predict.fit_predict(functionals=)) at config #3's tree, against the same fit_predict without functionals (the code path of
stm_mcmc_points: no functional step runs).  New points: the side x side grid offset by half a grid step;
functionals: one areal mean per 100 x 10 block of grid cells (1000 of 1000 cells each at side 1000) plus the mean over all
points.  Summaries only, nothing saved per draw; every iteration is saved (burn 0, thin 1), so fit milliseconds per iteration =
per saved iteration, and the chain is the same in both variants.  The two variants alternate, `rounds` times each.
    python profiles/micro/functionals_time.py [side] [keep] [grid_side] [rounds]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from spamtree_amd.model import functionals_csr  # noqa: E402
from spamtree_amd.predict import areal_means, fit_predict  # noqa: E402
from spamtree_amd.synthetic import make_workload  # noqa: E402


def setup(side, grid_side):
    wl = make_workload(side, device=0)
    g = (np.arange(grid_side) + 0.5) / (side - 1)          # the workload's grid step is 1 / (side - 1)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    Xn = np.random.default_rng(3).standard_normal((pts.shape[0], wl["p"]))
    i, j = np.divmod(np.arange(grid_side * grid_side), grid_side)
    labels = (i // 100) * -(-grid_side // 10) + j // 10    # blocks of 100 x 10 cells
    ptr, idx, wt = areal_means(labels)
    n = pts.shape[0]
    fun = (np.concatenate([ptr, [ptr[-1] + n]]), np.concatenate([idx, np.arange(n)]), np.concatenate([wt, np.full(n, 1.0 / n)]))
    return wl, pts, Xn, functionals_csr(fun, n)


def run(wl, pts, Xn, fun, keep):
    out = fit_predict(wl, pts, np.ones(pts.shape[0], dtype=np.int64), Xn, return_draws=False, functionals=fun, mcmc_keep=keep,
                      mcmc_burn=0, mcmc_thin=1, adapting=True, seed=11, device=0, save_w=False, save_yhat=False)
    return out, 1e3 * out["mcmc_time"] / keep


def main():
    a = [int(x) for x in sys.argv[1:]]
    side, keep, grid_side, rounds = (a + [1000, 50, 1000, 3][len(a):])[:4]
    wl, pts, Xn, fun = setup(side, grid_side)
    nf, nnz = fun[0].size - 1, fun[1].size
    print(f"n = {wl['n']}, {pts.shape[0]} new points, {nf} functionals, {nnz} terms, keep {keep}", flush=True)
    run(wl, pts, Xn, None, 3)            # warm-up: code objects, allocations
    run(wl, pts, Xn, fun, 3)
    base, feat = [], []
    for _ in range(rounds):
        ob, tb = run(wl, pts, Xn, None, keep)
        of, tf = run(wl, pts, Xn, fun, keep)
        base.append(tb)
        feat.append(tf)
        assert np.array_equal(ob["theta_mcmc"], of["theta_mcmc"]) and np.array_equal(ob["new"]["mean"], of["new"]["mean"])
    f = of["new"]["functionals"]
    # the functional over all points against the mean of the per-point summaries (a different summation order)
    check = abs(f["mean"][-1] - of["new"]["mean"].mean()) / max(1e-300, abs(of["new"]["mean"]).mean())
    alg = 16.0 * 2 * nnz + 8.0 * 4 * nnz     # terms of both lists; w, mean, yhat and var gathered once per term
    print(json.dumps(dict(ms_per_saved_iter_without=base, ms_per_saved_iter_with=feat,
                          added_ms_median=float(np.median(np.array(feat) - np.array(base))), n_fun=nf, terms=nnz,
                          alg_bytes_terms_and_gathers=alg, mean_all_rel_diff=check,
                          accepted=len({tuple(c) for c in of["theta_mcmc"].T}))), flush=True)


if __name__ == "__main__":
    main()
