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
parents / children) and the data of the sweep (y, XB, tausq per row).  WorkloadView supplies the same from the CSR arrays of
a workload (synthetic.make_workload), lazily per block, so that single blocks of full-size problems can be checked without
the float64 oracle model, which does not fit in memory there.

Besides the phase-A quantities and the sweep's conditional mean, the draws themselves are restated, each from the formula of
the code path it judges: cond_draw (the sweep, gibbs_sample_w), predict_draw (phase P, predict), prior_draw (st_simulate's
root-to-leaf sweep) and point_moments (the predictive at a new location, predict_points.hpp).
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


class _Csr:
    """Row u of a CSR pair (ptr, idx), or of a list of arrays, as an int64 array."""

    def __init__(self, x):
        if isinstance(x, tuple):
            self.ptr, self.idx = np.asarray(x[0], dtype=np.int64), np.asarray(x[1], dtype=np.int64)
            self.lists = None
        else:
            self.lists = [np.asarray(a, dtype=np.int64) for a in x]
            self.ptr = np.zeros(len(self.lists) + 1, dtype=np.int64)
            self.ptr[1:] = np.cumsum([a.size for a in self.lists])

    def __len__(self):
        return self.ptr.size - 1

    def __getitem__(self, u):
        if self.lists is not None:
            return self.lists[u]
        return self.idx[self.ptr[u]:self.ptr[u + 1]]

    def sizes(self):
        return np.diff(self.ptr)


class _ParentsIndexing:
    """parents_indexing[u] = the rows of u's parents in parent order, built on first use and cached."""

    def __init__(self, indexing, parents):
        self.indexing, self.parents = indexing, parents
        self._cache = {}

    def __getitem__(self, u):
        u = int(u)
        if u not in self._cache:
            par = self.parents[u]
            self._cache[u] = (np.concatenate([self.indexing[int(p)] for p in par]) if par.size
                              else np.zeros(0, dtype=np.int64))
        return self._cache[u]


class WorkloadView:
    """Index-only stand-in for the oracle model: what ExtendedBlocks reads, from a workload's arrays.

    wl: the dict of synthetic.make_workload (indexing / parents / children as (ptr, idx) CSR pairs) or of tests.util.make_problem
    (lists); Bcoeff: p x q (or p) regression coefficients, XB = X Bcoeff[:, outcome] per row; tausq_inv: q values (or one).
    As in the model, y is 0 at the rows without an observation and every row carries its outcome's tausq_inv."""

    def __init__(self, wl, Bcoeff, tausq_inv, limited_tree=False):
        self.q = int(wl["q"])
        self.coords = np.asarray(wl["coords"], dtype=np.float64)
        self.mv_id = np.asarray(wl["mv_id"], dtype=np.int64)
        self.block_groups = np.asarray(wl["block_groups"])
        self.res_is_ref = np.asarray(wl["res_is_ref"], dtype=np.int64)
        self.limited_tree = bool(limited_tree)
        self.indexing = _Csr(wl["indexing"])
        self.parents = _Csr(wl["parents"])
        self.children = _Csr(wl["children"])
        self.parents_indexing = _ParentsIndexing(self.indexing, self.parents)
        self.n_blocks = len(self.indexing)
        y = np.asarray(wl["y"], dtype=np.float64).reshape(-1)
        obs = np.isfinite(y)
        self.y = np.where(obs, y, 0.0)
        mv0 = self.mv_id - 1
        B = np.asarray(Bcoeff, dtype=np.float64)
        B = np.repeat(B.reshape(-1, 1), self.q, axis=1) if B.ndim == 1 else B
        X = np.asarray(wl["X"], dtype=np.float64)
        self.XB = np.zeros(y.size)
        for j in range(self.q):
            sel = mv0 == j
            self.XB[sel] = X[sel] @ B[:, j]
        self.tausq_inv = np.broadcast_to(np.asarray(tausq_inv, dtype=np.float64), (self.q,)).copy()
        self.tausq_inv_long = self.tausq_inv[mv0]
        rows = self.indexing.idx if self.indexing.lists is None else \
            np.concatenate(self.indexing.lists + [np.zeros(0, dtype=np.int64)])
        ct = np.concatenate([[0], np.cumsum(obs[rows])])
        self.block_ct_obs = ct[self.indexing.ptr[1:]] - ct[self.indexing.ptr[:-1]]


class ExtendedBlocks:
    """Per-block extended-precision results for one problem and theta, computed on demand and cached.

    om: an oracle model of the problem or a WorkloadView of it (only the index sets and data are read); theta: the covariance
    parameters.  block(u) -> dict(H, N, Ri (reference: m x m) or d (non-reference: m), logdet, rdiag (diagonal of R),
    min_pivot (min R pivot / max K_ii), isref)."""

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
            out.update(Ri=Ri, N=-(Ri @ H), logdet=np.sum(np.log(np.diag(Ri))), pivots=piv, rdiag=np.diag(R).copy())
        else:
            piv = np.diag(Kuu) - np.sum(V * V, axis=0)
            d = 1 / np.sqrt(piv)
            out.update(d=d, N=-(d[:, None] * H), logdet=np.sum(np.log(d)), pivots=piv, rdiag=piv)
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

    def _cond_system(self, b, w, w_desc=None):
        """(Q, rhs) of block b's full conditional given every other row of w: see cond_mean.  w_desc: where the rows of b's
        descendants themselves are read (default w)."""
        om = self.om
        ib = om.indexing[b]
        wl = np.asarray(w, dtype=LD)
        wd = wl if w_desc is None else np.asarray(w_desc, dtype=LD)
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
            resid = wd[om.indexing[c]] - Ho @ wl[om.parents_indexing[c][~cols]]
            rhs = rhs + Hb.T @ (Rc @ resid)
        return Q, rhs

    def cond_mean(self, b, w):
        """Mean of w over block b given every other row of w (float64, all rows), under the DAG precision
        Q = sum_u (E_u - H_u E_pa)' R_u^-1 (E_u - H_u E_pa) + diag(tausq_inv) (the data term as the sampler adds it, to
        every row of an observed block), with the linear term diag(tausq_inv) (y - XB), assembled from the terms that touch b: its own
        and those of its observed children."""
        Q, rhs = self._cond_system(b, w)
        L, _ = chol(Q)
        Li = inv_lower(L)
        return Li.T @ (Li @ rhs)

    def cond_draw(self, b, w, z, w_desc=None):
        """The sweep's draw of block b with the block's normals z (m): Li' (Li rhs + z) with Li = chol(Q)^-1 and (Q, rhs)
        those of cond_mean, which is the formula of gibbs_sample_w for a reference block.  The rows of a non-reference block
        are drawn one at a time from their own prior term and data term, as the sampler does (their observed descendants, if
        any, do not enter).

        What the sweep conditions b on: it runs leaf to root and forms a descendant c's message to its ancestors when it draws
        c, so the message carries c's new rows and the values c's other ancestors had then, i.e. before the sweep reached
        them.  So w holds the values before the sweep (b's ancestors, and every descendant's other ancestors) and w_desc those
        after it (the descendants' own rows; default w)."""
        z = np.asarray(z, dtype=LD)
        blk = self.block(b)
        if blk["isref"]:
            Q, rhs = self._cond_system(b, w, w_desc)
            Li = inv_lower(chol(Q)[0])
            return Li.T @ (Li @ rhs + z)
        om = self.om
        ib = om.indexing[b]
        tinv = np.asarray(om.tausq_inv_long[ib], dtype=LD)
        d2 = blk["d"] * blk["d"]
        mu = blk["H"] @ np.asarray(w, dtype=LD)[om.parents_indexing[b]] if blk["P"] else np.zeros(ib.size, dtype=LD)
        sc = 1 / np.sqrt(d2 + tinv)
        return sc * sc * (d2 * mu + tinv * np.asarray(om.y[ib] - om.XB[ib], dtype=LD)) + sc * z

    def predict_draw(self, u, w, z):
        """Phase P at a block without observations, row by row: H w_pa + sqrt(max(K_jj - V_j'V_j, 0)) z_j (z: the block's m
        normals)."""
        b = self.block(u)
        om = self.om
        mu = b["H"] @ np.asarray(w, dtype=LD)[om.parents_indexing[u]]
        return mu + np.sqrt(np.maximum(b["rdiag"], 0)) * np.asarray(z, dtype=LD)

    def prior_draw(self, u, w, z):
        """st_simulate's draw of block u given its parents' values in w: H w_pa + Ri^-1 z (reference) or z / d
        (non-reference)."""
        b = self.block(u)
        z = np.asarray(z, dtype=LD)
        e = inv_lower(b["Ri"]) @ z if b["isref"] else z / b["d"]
        if b["P"]:
            e = e + b["H"] @ np.asarray(w, dtype=LD)[self.om.parents_indexing[u]]
        return e

    def point_moments(self, anchor, coords, mv, w):
        """Conditional mean and variance of new points anchored at block `anchor` (coords k x 2, mv 1-based margins, w all
        rows): they condition on the chain root .. r of the reference block r = anchor (reference anchor) or its last parent,
        and with Linv_S its inverse Cholesky factor and k = K(S, x*):  v = Linv_S k, u = Linv_S w_S, mean = v'u,
        var = max(K(x*, x*) - v'v, 0)  (predict_points.hpp).  Full trees only."""
        om = self.om
        if om.limited_tree:
            raise ValueError("point_moments: full trees only")
        r = int(anchor) if self.isref[int(anchor)] else int(om.parents[int(anchor)][-1])
        rows, Li = self.chain_invchol(r)
        pts = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
        k = pts.shape[0]
        allc = np.vstack([self.coords[rows], pts])
        allv = np.concatenate([self.mv0[rows], np.asarray(mv, dtype=np.int64).reshape(-1) - 1])
        S, X = np.arange(rows.size), rows.size + np.arange(k)
        V = Li @ covariance(allc, allv, self.theta, self.q, S, X)
        u = Li @ np.asarray(w, dtype=LD)[rows]
        kxx = np.array([covariance(allc, allv, self.theta, self.q, X[i:i + 1], X[i:i + 1])[0, 0] for i in range(k)])
        return V.T @ u, np.maximum(kxx - np.sum(V * V, axis=0), 0)
