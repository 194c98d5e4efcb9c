"""Reference of the leave-group-out criteria (spamtree_amd/loo.py has the definition), for the tests, beside tests/loo_reference.py:
one group's draw in np.longdouble from its A = Q_GG and c = (Qw)_G (plain loops, an unpivoted Cholesky), the exact Gaussian
leave-group-out density log p(y_G | y_-G) at fixed theta, beta and tausq, and the labellings the tests use."""
import math

import numpy as np

from tests import loo_reference as lr

LD = np.longdouble


def chol_ld(A):
    """The unpivoted Cholesky factor of A in long double, or None when a pivot is not > 0."""
    A = np.array(A, dtype=LD)
    g = A.shape[0]
    L = np.zeros((g, g), dtype=LD)
    for k in range(g):
        p = A[k, k] - (L[k, :k] * L[k, :k]).sum()
        if not p > 0:
            return None
        L[k, k] = np.sqrt(p)
        for i in range(k + 1, g):
            L[i, k] = (A[i, k] - (L[i, :k] * L[k, :k]).sum()) / L[k, k]
    return L


def solve_lower_ld(L, b):
    b = np.array(b, dtype=LD)
    x = np.zeros_like(b)
    for i in range(L.shape[0]):
        x[i] = (b[i] - (L[i, :i] * x[:i].T).T.sum(axis=0)) / L[i, i]
    return x


def group_terms_ld(A, c, wG, yG, xbG, tausqG):
    """dict(l, phi, mu, obs, cond_mean, cond_cov, kappa_A, kappa_S, quad, sig) of one draw of one group in long double (Phi through
    float64 erfc: it only weights); l = NaN when a pivot is not > 0."""
    g = len(wG)
    ob = np.nonzero(np.isfinite(np.asarray(yG, dtype=np.float64)))[0]
    nan = float("nan")
    out = dict(l=LD(nan), phi=np.full(ob.size, nan), mu=np.full(ob.size, nan, dtype=LD), obs=ob, cond_mean=None, cond_cov=None,
               kappa_A=nan, kappa_S=nan, quad=nan, sig=None)
    if not np.all(np.isfinite(np.asarray(A, dtype=np.float64))):
        return out
    out["kappa_A"] = float(np.linalg.cond(np.asarray(A, dtype=np.float64)))
    L = chol_ld(A)
    if L is None:
        return out
    Li = solve_lower_ld(L, np.eye(g, dtype=LD))
    V = Li.T @ Li
    m = np.asarray(wG, dtype=LD) - V @ np.asarray(c, dtype=LD)
    mu = np.asarray(xbG, dtype=LD)[ob] + m[ob]
    Sig = V[np.ix_(ob, ob)] + np.diag(np.asarray(tausqG, dtype=LD)[ob])
    out.update(cond_mean=m, cond_cov=V, mu=mu, sig=np.sqrt(np.diag(Sig)).astype(np.float64))
    if not np.all(np.isfinite(Sig.astype(np.float64))):
        return out
    out["kappa_S"] = float(np.linalg.cond(Sig.astype(np.float64)))
    Ls = chol_ld(Sig)
    if Ls is None:
        return out
    r = np.asarray(yG, dtype=LD)[ob] - mu
    z = solve_lower_ld(Ls, r)
    quad = (z * z).sum()
    out["quad"] = float(quad)
    out["l"] = -quad / 2 - np.log(np.diag(Ls)).sum() - ob.size * np.log(2 * np.pi * LD(1)) / 2
    zs = (r / np.sqrt(np.diag(Sig))).astype(np.float64)
    out["phi"] = np.array([math.erfc(-v / math.sqrt(2.0)) / 2 for v in zs])
    return out


def exact_lgo(pb, Q, rows, xb, tausq_row, members):
    """log p(y_o | the other observed y) of every group at fixed theta, beta, tausq (o: the group's members with an observed y):
    y_obs ~ N(xb, C + diag(tausq)), C = Q^-1 on the rows of the density.  With P the precision of y_obs and r = y - xb:
    y_o | rest ~ N(y_o - P_oo^-1 (P r)_o, P_oo^-1)."""
    y = pb["y"]
    obs = np.nonzero(np.isfinite(y))[0]
    pos = -np.ones(y.size, dtype=np.int64)
    pos[obs] = np.arange(obs.size)
    C = np.zeros_like(Q)
    C[np.ix_(rows, rows)] = np.linalg.inv(Q[np.ix_(rows, rows)])
    Sig = C[np.ix_(obs, obs)] + np.diag(np.asarray(tausq_row, dtype=np.float64)[obs])
    P = np.linalg.inv(Sig)
    Pr = P @ (y[obs] - np.asarray(xb, dtype=np.float64)[obs])
    out = np.zeros(len(members))
    for g, m in enumerate(members):
        o = pos[m][pos[m] >= 0]
        Poo = P[np.ix_(o, o)]
        e = np.linalg.solve(Poo, Pr[o])
        out[g] = -0.5 * o.size * math.log(2 * math.pi) + 0.5 * np.linalg.slogdet(Poo)[1] - 0.5 * float(Pr[o] @ e)
    return out


def cell_labels(pb, k):
    """Labels of k x k cells of grid points: the grid's distinct coordinates ranked per axis, the ranks divided by k."""
    xy = pb["coords"][:, :2]
    ix = np.searchsorted(np.unique(xy[:, 0]), xy[:, 0]) // k
    iy = np.searchsorted(np.unique(xy[:, 1]), xy[:, 1]) // k
    return (ix * (iy.max() + 1) + iy).astype(np.int64)


def random_labels(n, size, seed):
    """Groups of `size` rows drawn without regard to the tree (members on different branches give structural zeros); a fifth of the
    rows in no group."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    lab = -np.ones(n, dtype=np.int64)
    used = perm[: (4 * n) // 5]
    lab[used] = np.arange(used.size) // size
    return lab
