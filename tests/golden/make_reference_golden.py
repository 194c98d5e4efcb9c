#!/usr/bin/env python3
"""Records fixtures from the COMPILED REFERENCE (oracle/_ref/libspamtree_ref.so: the reference's own covariance_functions.cpp,
mh_adapt.{h,cpp} and list_mean.cpp, built by oracle/Makefile) into tests/golden/ref_*.npz.

Unlike the vectors of make_golden.py (outputs of this repository's oracle), what these files hold next to their inputs are
outputs of reference source.  They are data only; each file stays under 300 KB (symmetric matrices are stored as their upper
triangle, row by row).  tests/test_gpu_reference_binary.py reads them on a machine that has neither the reference tree nor
the library; tests/test_reference_binary.py regenerates every array in memory and requires the committed bytes.

Run from the repo root, after `make -C oracle`:  python tests/golden/make_reference_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.util import distinct_theta, make_problem, nice_theta  # noqa: E402

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
MH_START = np.full(4, 0.5 * (1e-3 + 1e3))              # the Metropolis start value: midpoint of the prior bounds (phi ~ 500)

# ---- 1. CrossCovarianceAG10 --------------------------------------------------------------------------------------------
N1, N2, N_COINCIDENT = 60, 50, 5


def crosscov_theta(q, zero_d=False):
    """Every per-outcome parameter and every Dmat entry different, ai1 of mixed sign."""
    ai1 = np.array([1.0, -0.8, 1.3, 0.9, -1.1, 0.7])[:q]
    ai2 = np.array([0.31, 0.52, 0.44, 0.67, 0.23, 0.58])[:q]
    phi = np.array([3.0, 4.5, 2.2, 5.1, 3.7, 6.3])[:q]
    thetamv = np.array([1.2, 0.7, 4.0]) if q > 2 else np.array([5.0])
    k = q * (q - 1) // 2
    dvec = 0.4 + 0.17 * np.arange(1, k + 1) ** 1.3
    if zero_d:
        dvec[1] = 0.0                                   # Dmat[2, 0] = Dmat[0, 2] = 0 between DIFFERENT outcomes
    return np.concatenate([ai1, ai2, phi, thetamv, dvec])


def crosscov_inputs(name, q):
    rng = np.random.default_rng(1000 + 10 * q + (1 if name.endswith("zeroD") else 0))
    c1, c2 = rng.uniform(size=(N1, 2)), rng.uniform(size=(N2, 2))
    m1 = np.concatenate([np.arange(1, q + 1), rng.integers(1, q + 1, N1 - q)])
    m2 = np.concatenate([np.arange(q, 0, -1), rng.integers(1, q + 1, N2 - q)])
    hit = rng.choice(N1, N_COINCIDENT, replace=False)
    c2[7:7 + N_COINCIDENT] = c1[hit]                    # h = 0, between equal and between different outcomes
    return c1, m1.astype(np.int64), c2, m2.astype(np.int64)


CROSSCOV_CASES = [("q2", 2, False), ("q3", 3, False), ("q4", 4, False), ("q5", 5, False), ("q6", 6, False),
                  ("q3_zeroD", 3, True)]


def rd_example():
    """man/CrossCovarianceAG10.Rd:72-93, as tests/test_gpu_parity.py::test_cross_covariance_ag10_export builds it."""
    xl = np.linspace(0.0, 1.0, 10)
    g = np.array([(a, b) for b in xl for a in xl])
    return dict(cx=np.vstack([g, g]), mv=np.repeat([1, 2], 100).astype(np.int64), ai1=np.array([1, 1.5]),
                ai2=np.array([.1, .51]), phi_i=np.array([1.0, 2.0]), thetamv=np.array([5.0]), Dmat=np.array([[0, 1.0], [1.0, 0]]))


def upper(K):
    assert np.array_equal(K, K.T)
    return K[np.triu_indices(K.shape[0])].copy()


def from_upper(v, n):
    K = np.zeros((n, n))
    K[np.triu_indices(n)] = v
    return K + np.triu(K, 1).T


def build_crosscov(lib):
    d = {"cases": np.array([c[0] for c in CROSSCOV_CASES])}
    for name, q, zero_d in CROSSCOV_CASES:
        theta = crosscov_theta(q, zero_d)
        t = lib.transform(q, theta)                     # the reference's own slicing and Dmat fill
        c1, m1, c2, m2 = crosscov_inputs(name, q)
        out = lib.CrossCovarianceAG10(c1, m1, c2, m2, t["ai1"], t["ai2"], t["phi_i"], t["thetamv"], t["Dmat"])
        for k, v in dict(theta=theta, coords1=c1, mv1=m1, coords2=c2, mv2=m2, ai1=t["ai1"], ai2=t["ai2"], phi_i=t["phi_i"],
                         thetamv=t["thetamv"], Dmat=t["Dmat"], out=out).items():
            d[f"{name}_{k}"] = v
    return d


def build_crosscov_rd(lib):
    e = rd_example()
    out = lib.CrossCovarianceAG10(e["cx"], e["mv"], e["cx"], e["mv"], e["ai1"], e["ai2"], e["phi_i"], e["thetamv"], e["Dmat"])
    return dict(e, out_upper=upper(out))


# ---- 2. dense Covariancef(same = true) of whole small problems -----------------------------------------------------------
# multi-level trees (three levels each) with blocks of at most 32 rows, and two one-level trees for the exact-GP identity
DENSE = {
    "q1_grid": (dict(side=12, q=1, seed=5), {"nice": nice_theta(1), "mh_start": MH_START}),
    "q1_random": (dict(side=12, q=1, seed=5, random_coords=True), {"nice": nice_theta(1), "mh_start": MH_START}),
    "q2": (dict(side=10, q=2, seed=5, cell_size=16), {"nice": nice_theta(2)}),
    "q3": (dict(side=8, q=3, seed=5, cell_size=9), {"distinct": distinct_theta(3)}),
    "q5": (dict(side=6, q=5, seed=5, cell_size=4), {"distinct": distinct_theta(5)}),
    "onelevel": (dict(side=5, q=1, seed=3), {"nice": nice_theta(1)}),
    "onelevel_q3": (dict(side=5, q=3, seed=3), {"distinct": distinct_theta(3)}),
}


def build_dense(lib, name):
    kw, thetas = DENSE[name]
    pb = make_problem(**kw)
    n, q = pb["n"], pb["q"]
    assert n <= 250
    rows = np.arange(n)
    d = dict(kw=np.array(json.dumps(kw, sort_keys=True)), coords=pb["coords"], mv_id=np.asarray(pb["mv_id"], dtype=np.int64),
             theta_names=np.array(list(thetas)))
    for tname, theta in thetas.items():
        K = lib.Covariancef(q, theta, pb["coords"], pb["mv_id"] - 1, rows, rows, True)
        d[f"theta_{tname}"] = np.asarray(theta, dtype=np.float64)
        d[f"K_upper_{tname}"] = upper(K)
    return d


# ---- 3. list_qtile / list_mean --------------------------------------------------------------------------------------------
KEEPS = (1, 2, 7, 40)
SUMMARY_ROWS = 64
REQUIRED_QS = (0.0, 0.025, 0.25, 0.5, 0.975, 1.0)


def qtile_r(q, keep):
    return ((q * 100.0) / 100.0) * keep                  # list_mean.cpp: cqtile passes q * 100, prctile_stl divides again


def landing_qs(keep):
    """One q whose r lands exactly on an integer and one whose r lands exactly on a half-integer (in the reference's own
    arithmetic), the smallest such numerators."""
    whole = next(k / keep for k in range(1, keep + 1) if qtile_r(k / keep, keep) == k)
    half = next((k + 0.5) / keep for k in range(keep) if qtile_r((k + 0.5) / keep, keep) == k + 0.5)
    return whole, half


def summary_draws(keep):
    """keep draws of a 64-row column; rows cycle through: distinct values, heavy ties, constant, mixed sign with repeats."""
    rng = np.random.default_rng(400 + keep)
    d = np.zeros((keep, SUMMARY_ROWS))
    for i in range(SUMMARY_ROWS):
        kind = i % 4
        if kind == 0:
            d[:, i] = (1.0 + i) * 0.37 * rng.permutation(keep) - 3.0
        elif kind == 1:
            d[:, i] = rng.integers(0, 3, keep) * 1.5 - 1.5
        elif kind == 2:
            d[:, i] = -2.75 + i
        else:
            d[:, i] = np.round(rng.standard_normal(keep), 1)          # repeats among 40 draws rounded to one decimal
    return d + 0.0            # no -0.0: it ties with +0.0, and which of the two a selection returns is the algorithm's choice


def build_summaries(lib):
    d = {"keeps": np.array(KEEPS, dtype=np.int64)}
    for keep in KEEPS:
        draws = summary_draws(keep)
        qs = np.array(sorted(set(REQUIRED_QS + landing_qs(keep))))
        x = [draws[i].reshape(-1, 1) for i in range(keep)]
        d[f"draws_{keep}"] = draws
        d[f"qs_{keep}"] = qs
        d[f"landing_{keep}"] = np.array(landing_qs(keep))
        d[f"qtile_{keep}"] = np.stack([lib.list_qtile(x, q).reshape(-1) for q in qs])
        d[f"mean_{keep}"] = lib.list_mean(x).reshape(-1)
    return d


# ---- 4. RAMAdapt trajectories ---------------------------------------------------------------------------------------------
RAM_STEPS = 120
RAM_PS = (4, 10, 21)                                     # theta of q = 1, 3, 6


def ram_inputs(p):
    rng = np.random.default_rng(700 + p)
    A = 0.05 * (np.eye(p) + 0.1 * rng.standard_normal((p, p)))
    S0 = A @ A.T
    U = rng.standard_normal((RAM_STEPS, p))
    accept = rng.uniform(size=RAM_STEPS) < 0.35
    accept[20:34] = False                                 # runs of rejections, before and after the start of adaptation
    accept[70:85] = False
    alpha = np.where(accept, np.minimum(1.5, rng.uniform(0.2, 1.6, RAM_STEPS)), rng.uniform(0.0, 0.3, RAM_STEPS))
    alpha[75:80] = 0.0                                    # proposals that were not acceptable
    alpha[90] = np.nan                                    # exp(nan log-ratio): the reference's std::min(1.0, alpha) gives 1
    alpha[95] = np.inf
    return S0, U, alpha, accept


def run_ram(ram, U, alpha, accept):
    """The call sequence of one Metropolis step (spamtree_fit.cpp) for every step; paramsd, S, started, accept_ratio after each."""
    p = U.shape[1]
    P, S = np.zeros((RAM_STEPS, p, p)), np.zeros((RAM_STEPS, p, p))
    started, ratio = np.zeros(RAM_STEPS, dtype=np.int64), np.zeros(RAM_STEPS)
    for mc in range(RAM_STEPS):
        ram.count_proposal()
        if accept[mc]:
            ram.count_accepted()
        ram.update_ratios()
        ram.adapt(U[mc], float(alpha[mc]), mc)
        P[mc], S[mc], started[mc], ratio[mc] = ram.paramsd, ram.S, int(ram.started), ram.accept_ratio
    return P, S, started, ratio


def build_ram(lib, p):
    S0, U, alpha, accept = ram_inputs(p)
    P, S, started, ratio = run_ram(lib.RAMAdapt(p, S0), U, alpha, accept)
    # from the switch on paramsd is a lower Cholesky factor; before it, it is the constructor's: the lower triangle holds it
    assert np.all(np.triu(P, 1)[started == 1] == 0.0) and np.all(P[started == 0] == P[0])
    low = np.tril_indices(p)
    return dict(S0=S0, U=U, alpha=alpha, accept=accept.astype(np.int64), paramsd_lower=P[:, low[0], low[1]].copy(),
                started=started, accept_ratio=ratio)


def build_all(lib):
    files = {"ref_crosscov": build_crosscov(lib), "ref_crosscov_rd": build_crosscov_rd(lib), "ref_summaries": build_summaries(lib)}
    for name in DENSE:
        files[f"ref_dense_{name}"] = build_dense(lib, name)
    for p in RAM_PS:
        files[f"ref_ramadapt_p{p}"] = build_ram(lib, p)
    return files


def main():
    from oracle import reflib
    lib = reflib.load()
    if lib is None:
        sys.exit("oracle/_ref/libspamtree_ref.so is missing: run `make -C oracle` where the reference tree exists")
    for name, d in build_all(lib).items():
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(f"{name}: {len(d)} arrays, {size} bytes")
        assert size < 300 * 1024, name


if __name__ == "__main__":
    main()
