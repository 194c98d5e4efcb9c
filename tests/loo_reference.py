"""Reference of the leave-one-out criteria with the latent field integrated out (spamtree_amd/loo.py has the definition), for the
tests: the DAG's prior precision from the dense covariance matrix (nothing of the oracle's per-block caches, nothing of the device),
the conditional moments, the accumulation and the finish in np.longdouble, and the exact Gaussian leave-one-out density at fixed
theta, beta and tausq."""
import math

import numpy as np

from oracle import spamtree_oracle as so

LD = np.longdouble
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def dense_cov(pb, theta):
    cp = so.CovarianceParams(2, pb["q"], -1)
    cp.transform(theta)
    rows = np.arange(pb["n"])
    return so.Covariancef(pb["coords"], pb["mv_id"] - 1, rows, rows, cp, True)


def density_blocks(pb):
    """The blocks that take part in the density the sampler targets: those with an observed row."""
    return [u for u in range(len(pb["indexing"])) if np.isfinite(pb["y"][pb["indexing"][u]]).any()]


def density_precision(pb, theta):
    """(Q, rows): Q = sum over the blocks with observed rows of (I_u - H_u E_pa)' R_u^-1 (I_u - H_u E_pa), R_u diagonal on
    non-reference levels (the observed-blocks loop of tests/test_oracle_identities.py::test_loglik_equals_dense_dag_density), n x n
    with zero rows and columns at the prediction blocks; rows = the rows of the density, ascending."""
    n = pb["n"]
    K = dense_cov(pb, theta)
    Q = np.zeros((n, n))
    labels = np.unique(pb["block_groups"])
    blocks = density_blocks(pb)
    for u in blocks:
        iu = pb["indexing"][u]
        pa = pb["parents"][u]
        g = int(np.nonzero(labels == pb["block_groups"][u])[0][0])
        B = np.zeros((iu.size, n))
        B[np.arange(iu.size), iu] = 1.0
        if pa.size:
            pi = np.concatenate([pb["indexing"][a] for a in pa])
            H = np.linalg.solve(K[np.ix_(pi, pi)], K[np.ix_(pi, iu)]).T
            B[:, pi] -= H
            R = K[np.ix_(iu, iu)] - H @ K[np.ix_(pi, iu)]
        else:
            R = K[np.ix_(iu, iu)]
        if pb["res_is_ref"][g] == 0:
            R = np.diag(np.diag(R))
        Q += B.T @ np.linalg.solve(R, B)
    return Q, np.sort(np.concatenate([pb["indexing"][u] for u in blocks]))


def moments(Q, w, rows):
    """dict(q_diag, qw, cond_mean, cond_var) in float64 from a long-double product; NaN off `rows`."""
    n = Q.shape[0]
    d = np.diag(Q).astype(LD)
    c = Q.astype(LD) @ np.asarray(w, dtype=LD)
    out = {k: np.full(n, np.nan) for k in ("q_diag", "qw", "cond_mean", "cond_var")}
    out["q_diag"][rows] = d[rows]
    out["qw"][rows] = c[rows]
    out["cond_mean"][rows] = (np.asarray(w, dtype=LD)[rows] - c[rows] / d[rows])
    out["cond_var"][rows] = (1 / d[rows])
    return out


def draw_terms_ld(y, xb, cond_mean, cond_var, tausq):
    """(l, Phi, mu) of one draw per row in long double (Phi through float64 erfc: it only weights)."""
    mu = np.asarray(xb, dtype=LD) + np.asarray(cond_mean, dtype=LD)
    with np.errstate(all="ignore"):
        s2 = np.asarray(cond_var, dtype=LD) + np.asarray(tausq, dtype=LD)
        z = (np.asarray(y, dtype=LD) - mu) / np.sqrt(s2)
        l = -z * z / 2 - np.log(s2) / 2 - np.log(2 * np.pi * LD(1)) / 2
    zf = np.where(np.isfinite(z), z, 0.0).astype(np.float64)
    return l, (_erfc(-zf / math.sqrt(2.0)) / 2).astype(LD), mu


def estimator_ld(ls, phis, mus):
    """The four outputs and the weights' relative standard error from S x n arrays of l, Phi, mu (long double, direct sums with
    the maximum taken out); draws with a non-finite l are left out of a row.  Returns (dict, n_skipped, se)."""
    ls, phis, mus = (np.asarray(a, dtype=LD) for a in (ls, phis, mus))
    ok = np.isfinite(ls)
    t = np.where(ok, -ls, -np.inf)
    with np.errstate(all="ignore"):
        M = t.max(axis=0)
        x = np.where(ok, np.exp(t - M), 0)
        Si = ok.sum(axis=0).astype(LD)
        A1, A2 = x.sum(axis=0), (x * x).sum(axis=0)
        out = dict(elpd_loo=-(M + np.log(A1 / Si)), pit_loo=(x * np.where(ok, phis, 0)).sum(axis=0) / A1,
                   mu_loo=(x * np.where(ok, mus, 0)).sum(axis=0) / A1, weight_ess=A1 * A1 / A2)
        mean = A1 / Si
        sd = np.sqrt(np.maximum(A2 / Si - mean * mean, 0) * Si / np.maximum(Si - 1, 1))
        se = sd / mean / np.sqrt(Si)
    out = {k: np.where(Si > 0, v, np.nan).astype(np.float64) for k, v in out.items()}
    return out, int((~ok).sum()), se.astype(np.float64)


def exact_loo(pb, Q, rows, xb, tausq_row):
    """log p(y_i | y_-i) of every observed row at fixed theta, beta, tausq: y_obs ~ N(xb, C + diag(tausq)), C the DAG's covariance
    of the observed rows = (Q^-1) there.  With P = (C + T)^-1 and r = y - xb: y_i | y_-i ~ N(y_i - (P r)_i / P_ii, 1 / P_ii).
    NaN off the observed rows."""
    y = pb["y"]
    obs = np.nonzero(np.isfinite(y))[0]
    C = np.zeros_like(Q)
    C[np.ix_(rows, rows)] = np.linalg.inv(Q[np.ix_(rows, rows)])
    Sig = C[np.ix_(obs, obs)] + np.diag(np.asarray(tausq_row, dtype=np.float64)[obs])
    P = np.linalg.inv(Sig)
    r = y[obs] - np.asarray(xb, dtype=np.float64)[obs]
    pd = np.diag(P)
    e = (P @ r) / pd
    out = np.full(y.size, np.nan)
    out[obs] = -0.5 * math.log(2 * math.pi) + 0.5 * np.log(pd) - 0.5 * e * e * pd
    return out


def posterior_w(pb, Q, rows, xb, tausq_row):
    """(mean, chol of the covariance) of w | y over `rows` at fixed theta, beta, tausq: precision Q + diag(1 / tausq at observed)."""
    y = pb["y"]
    obs = np.isfinite(y)
    D = np.where(obs, 1.0 / np.asarray(tausq_row, dtype=np.float64), 0.0)
    A = Q[np.ix_(rows, rows)] + np.diag(D[rows])
    V = np.linalg.inv(A)
    V = (V + V.T) / 2
    b = np.where(obs, (np.where(obs, y, 0.0) - np.asarray(xb, dtype=np.float64)) * D, 0.0)[rows]
    return V @ b, np.linalg.cholesky(V)
