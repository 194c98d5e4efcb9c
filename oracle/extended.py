"""Extended-precision per-block reference (CPU only): the phase-A quantities of every block and the sweep's full conditional
means, restated from their definitions in 80-bit long double.

The float64 oracle keeps about 6 significant digits of Ri and of the panel N = -Ri H when phi is at the bottom of its bounds
(phi = 1e-3: K_pa is nearly singular and R = K_uu - V'V cancels), so it cannot judge a kernel there.  This module recomputes
the same quantities from the float64 coordinates and theta with nothing but long-double arithmetic: the covariance by its
closed form, a plain column Cholesky and triangular inverse (no LAPACK), and per block u with ancestors pa:

    V = L_pa^-1 K_pa,u,  H = V' L_pa^-1 = K_u,pa K_pa^-1,  R = K_uu - V'V,
    reference block:      Ri = chol(R)^-1, N = -Ri H, logdet component = sum log diag Ri
    non-reference block:  d_i = 1 / sqrt(R_ii), N = -diag(d) H, logdet component = sum log d_i

L_pa^-1, the inverse Cholesky factor of the chain pa = (ancestors of u), is assembled block by block from the ancestors' own
results ([[L_pa'^-1, 0], [N_a, Ri_a]] for the last ancestor a), which is the definition of a block inverse Cholesky factor,
and cached per last ancestor.  The only things taken from the oracle model are the index sets (indexing, parents_indexing,
parents / children) and the data of the sweep (y, XB, tausq per row).
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise ImportError(f"oracle.extended needs an extended-precision long double (eps <= 1e-18); this platform's long double "
                      f"has eps = {float(np.finfo(LD).eps):.3g}.  Refusing to run in float64 precision.")

HL2PI = -LD("0.918938533204672741780329736405617639861")   # -log(2 pi) / 2


def chol(A):
    """Lower Cholesky factor by columns; returns (L, pivots d_j = L_jj^2).  A non-positive pivot gives NaN from there on."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    d = np.zeros(n, dtype=LD)
    for j in range(n):
        d[j] = A[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d[j]) if d[j] > 0 else LD("nan")
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, d


def inv_lower(L):
    """Inverse of a lower-triangular matrix by forward substitution, row by row."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = 1 / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def unpack_theta(theta, q):
    """theta -> (ai1, ai2, phi_i, thetamv, Dmat) in the layout of covariance_functions.cpp (CovarianceParams::transform)."""
    theta = np.asarray(theta, dtype=np.float64)
    n_cbase = 3 if q > 2 else 1
    npars = 3 * q + n_cbase
    ai1, ai2, phi = theta[:q], theta[q:2 * q], theta[2 * q:3 * q]
    tmv = theta[3 * q:npars]
    D = np.zeros((q, q))
    if q > 1:
        ix = 0
        for j in range(q):                       # column-wise fill of the strict lower triangle, then symmetric
            for i in range(j + 1, q):
                D[i, j] = D[j, i] = theta[npars + ix]
                ix += 1
    return ai1, ai2, phi, tmv, D


def covariance(coords, mv0, theta, q, i1, i2):
    """K[i1, i2] in long double: q = 1 sigma^2 exp(-phi h); q >= 2 the Apanasovich-Genton form of mvCovAG20107 (mv0: 0-based
    outcome of every row).  h = sqrt(dx^2 + dy^2) from the float64 coordinates."""
    c1 = np.asarray(coords[i1], dtype=LD)
    c2 = np.asarray(coords[i2], dtype=LD)
    dx = c1[:, 0][:, None] - c2[:, 0][None, :]
    dy = c1[:, 1][:, None] - c2[:, 1][None, :]
    h = np.sqrt(dx * dx + dy * dy)
    if q == 1:
        return LD(theta[0]) * np.exp(-LD(theta[3]) * h)
    ai1, ai2, phi, tmv, D = (np.asarray(a, dtype=LD) for a in unpack_theta(theta, q))
    v1, v2 = mv0[i1], mv0[i2]
    v = D[np.ix_(v1, v2)]
    if q > 2:
        psi = np.exp(LD(0.5) * tmv[1] * np.log1p(tmv[0] * v))          # (a v + 1)^(beta / 2)
        cb = np.exp(-tmv[2] * h / psi) / (psi * psi)
    else:
        psi = np.sqrt(v + 1)
        cb = np.exp(-tmv[0] * h / psi) / (v + 1)
    a1i, a1j = ai1[v1][:, None], ai1[v2][None, :]
    same = a1i * a1i * cb + ai2[v1][:, None] ** 2 * np.exp(-phi[v1][:, None] * h)
    return np.where(v == 0, same, a1i * a1j * cb)


class ExtendedBlocks:
    """Per-block extended-precision results for one problem and theta, computed on demand and cached.

    om: an oracle model of the problem (only its index sets and data are read); theta: the covariance parameters.
    block(u) -> dict(H, R, N, Ri (reference: m x m) or d (non-reference: m), logdet, min_pivot (min R pivot / max K_ii),
    isref)."""

    def __init__(self, om, theta):
        self.om = om
        self.theta = np.asarray(theta, dtype=np.float64)
        self.q = int(om.q)
        self.coords = np.asarray(om.coords, dtype=np.float64)
        self.mv0 = np.asarray(om.mv_id, dtype=np.int64) - 1
        grp = np.asarray(om.block_groups)
        labels = np.unique(grp)
        self.level = np.searchsorted(labels, grp)
        self.isref = np.asarray(om.res_is_ref)[self.level] == 1
        self._blk = {}
        self._chain = {}

    def cov(self, i1, i2):
        return covariance(self.coords, self.mv0, self.theta, self.q, i1, i2)

    def chain_invchol(self, a):
        """(rows, inverse Cholesky factor of K over them): the conditioning chain of a's children, rows = (a's ancestors'
        rows in parent order, a's rows), or a's rows alone in a limited tree."""
        if a not in self._chain:
            om = self.om
            b = self.block(a)
            if b["P"] == 0:
                rows, Li = om.indexing[a], b["Ri"]
            elif om.limited_tree:
                rows = om.indexing[a]
                Li = inv_lower(chol(self.cov(rows, rows))[0])
            else:
                prow, Lp = self.chain_invchol(int(om.parents[a][-1]))
                assert np.array_equal(prow, om.parents_indexing[a]), a
                rows = np.concatenate([prow, om.indexing[a]])
                P, m = b["P"], b["m"]
                Li = np.zeros((P + m, P + m), dtype=LD)
                Li[:P, :P] = Lp
                Li[P:, :P] = b["N"]
                Li[P:, P:] = b["Ri"]
            self._chain[a] = (rows, Li)
        return self._chain[a]

    def block(self, u):
        if u in self._blk:
            return self._blk[u]
        om = self.om
        iu = om.indexing[u]
        pa = om.parents_indexing[u]
        m, P = iu.size, pa.size
        Kuu = self.cov(iu, iu)
        if P:
            rows, Li = self.chain_invchol(int(om.parents[u][-1]))
            # the panel's column order is the chain's row order, element by element
            assert np.array_equal(rows, pa), u
            V = Li @ self.cov(pa, iu)
            H = V.T @ Li
        else:
            V = np.zeros((0, m), dtype=LD)
            H = np.zeros((m, 0), dtype=LD)
        isref = bool(self.isref[u]) or P == 0
        out = dict(m=m, P=P, H=H, isref=isref)
        if isref:
            R = Kuu - V.T @ V
            L, piv = chol(R)
            Ri = inv_lower(L)
            out.update(Ri=Ri, N=-(Ri @ H), logdet=np.sum(np.log(np.diag(Ri))), pivots=piv)
        else:
            piv = np.diag(Kuu) - np.sum(V * V, axis=0)
            d = 1 / np.sqrt(piv)
            out.update(d=d, N=-(d[:, None] * H), logdet=np.sum(np.log(d)), pivots=piv)
        out["min_pivot"] = float(np.min(piv) / np.max(np.diag(Kuu)))
        self._blk[u] = out
        return out

    def loglik_comp(self, u, w):
        """(logdet component, quadratic component m HL2PI - wx' R^-1 wx / 2) of block u at latent values w (float64, all rows)."""
        b = self.block(u)
        om = self.om
        wx = np.asarray(w[om.indexing[u]], dtype=LD)
        if b["P"]:
            wx = wx - b["H"] @ np.asarray(w[om.parents_indexing[u]], dtype=LD)
        core = np.sum((b["Ri"] @ wx) ** 2) if b["isref"] else np.sum((b["d"] * wx) ** 2)
        return b["logdet"], b["m"] * HL2PI - core / 2

    def prec(self, u):
        """R_u^-1."""
        b = self.block(u)
        return b["Ri"].T @ b["Ri"] if b["isref"] else np.diag(b["d"] * b["d"])

    def cond_mean(self, b, w):
        """Mean of w over block b given every other row of w (float64, all rows), under the DAG precision
        Q = sum_u (E_u - H_u E_pa)' R_u^-1 (E_u - H_u E_pa) + diag(tausq_inv) (the data term as the sampler adds it, to
        every row of an observed block), with the linear term diag(tausq_inv) (y - XB), assembled from the terms that touch b: its own
        and those of its observed children."""
        om = self.om
        ib = om.indexing[b]
        wl = np.asarray(w, dtype=LD)
        tinv = np.asarray(om.tausq_inv_long[ib], dtype=LD)      # as the sampler adds it: every row of an observed block
        Rb = self.prec(b)
        Q = Rb + np.diag(tinv)
        rhs = tinv * np.asarray(om.y[ib] - om.XB[ib], dtype=LD)
        blk = self.block(b)
        if blk["P"]:
            rhs = rhs + Rb @ (blk["H"] @ wl[om.parents_indexing[b]])
        for c in om.children[b]:
            c = int(c)
            if om.block_ct_obs[c] == 0:
                continue
            bc = self.block(c)
            off = 0
            for p in om.parents[c]:
                if int(p) == b:
                    break
                off += om.indexing[int(p)].size
            cols = np.zeros(bc["P"], dtype=bool)
            cols[off:off + ib.size] = True
            Hb, Ho = bc["H"][:, cols], bc["H"][:, ~cols]
            Rc = self.prec(c)
            Q = Q + Hb.T @ Rc @ Hb
            resid = wl[om.indexing[c]] - Ho @ wl[om.parents_indexing[c][~cols]]
            rhs = rhs + Hb.T @ (Rc @ resid)
        L, _ = chol(Q)
        Li = inv_lower(L)
        return Li.T @ (Li @ rhs)
