"""ORACLE -- test infrastructure only.  ctypes loader for oracle/_ref/libspamtree_ref.so: the reference's OWN
covariance_functions.cpp, mh_adapt.{h,cpp}, list_mean.cpp and find_nan.cpp, compiled unchanged by oracle/Makefile against the
stand-in oracle/refshim/RcppArmadillo.h, behind the C entry points of oracle/ref_capi.cpp.

load() returns None where the library has not been built (no reference tree at build time); callers decide what that means.
Everything here marshals arrays and nothing else: no formula of the reference is restated in this file.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(ROOT, "_ref", "libspamtree_ref.so")
DEFAULT_REF = "/root/reference"            # oracle/Makefile's REF

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
_cached = []


class ReferenceError_(RuntimeError):
    """The reference threw or stopped (code -1), or asked for a uniform the caller had not queued (-2)."""


def _f(a):
    return np.asfortranarray(a, dtype=np.float64).copy(order="F")


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _d(a):
    return a.ctypes.data_as(_dp)


def _l(a):
    return a.ctypes.data_as(_ip)


def reference_tree_present(ref=None):
    ref = ref or os.environ.get("REF", DEFAULT_REF)
    return os.path.exists(os.path.join(ref, "src", "covariance_functions.cpp"))


def _check(rc, what):
    if rc != 0:
        raise ReferenceError_(f"{what}: code {rc}")


class RefRAMAdapt:
    """The reference's RAMAdapt object (mh_adapt.h) behind a handle."""

    def __init__(self, lib, npars, metropolis_sd):
        self._l = lib
        self.p = int(npars)
        self._h = lib.ref_ram_create(self.p, _d(_f(metropolis_sd)))
        if not self._h:
            raise ReferenceError_("RAMAdapt constructor threw")

    def close(self):
        if self._h:
            self._l.ref_ram_destroy(self._h)
            self._h = None

    __del__ = close

    def count_proposal(self):
        self._l.ref_ram_count_proposal(self._h)

    def count_accepted(self):
        self._l.ref_ram_count_accepted(self._h)

    def update_ratios(self):
        self._l.ref_ram_update_ratios(self._h)

    def adapt(self, U, alpha, mc):
        _check(self._l.ref_ram_adapt(self._h, _d(_f(U)), float(alpha), int(mc)), "RAMAdapt::adapt")

    def _mat(self, fn):
        out = np.zeros((self.p, self.p), order="F")
        fn(self._h, _d(out))
        return out

    @property
    def paramsd(self):
        return self._mat(self._l.ref_ram_paramsd)

    @property
    def S(self):
        return self._mat(self._l.ref_ram_S)

    @property
    def started(self):
        return bool(self._l.ref_ram_started(self._h))

    @property
    def accept_ratio(self):
        return float(self._l.ref_ram_accept_ratio(self._h))

    @property
    def g0(self):
        return int(self._l.ref_ram_g0(self._h))


class RefLib:
    def __init__(self, path):
        lib = self._l = C.CDLL(path)
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        pi = C.POINTER(C.c_int)
        sigs = {
            "ref_transform": (ci, [ci, _dp, ci, _dp, _dp, _dp, _dp, _dp, pi]),
            "ref_vec_to_symmat": (ci, [_dp, ci, _dp, pi]),
            "ref_covariancef": (ci, [ci, ci, _dp, ci, _dp, ci, _ip, _ip, ci, _ip, ci, ci, _dp]),
            "ref_cross_covariance_ag10": (ci, [_dp, ci, _ip, _dp, ci, _ip, _dp, _dp, _dp, ci, _dp, ci, _dp, ci, _dp]),
            "ref_par_huvtransf_fwd": (ci, [_dp, ci, _dp, _dp]),
            "ref_par_huvtransf_back": (ci, [_dp, ci, _dp, _dp]),
            "ref_unif_bounds": (ci, [_dp, ci, _dp, pi]),
            "ref_calc_jacobian": (ci, [_dp, _dp, ci, _dp, _dp]),
            "ref_runif_push": (None, [_dp, ci]),
            "ref_runif_pending": (ci, []),
            "ref_runif_clear": (None, []),
            "ref_do_I_accept": (ci, [cd, pi]),
            "ref_ram_create": (vp, [ci, _dp]),
            "ref_ram_destroy": (None, [vp]),
            "ref_ram_count_proposal": (None, [vp]),
            "ref_ram_count_accepted": (None, [vp]),
            "ref_ram_update_ratios": (None, [vp]),
            "ref_ram_adapt": (ci, [vp, _dp, cd, ci]),
            "ref_ram_paramsd": (None, [vp, _dp]),
            "ref_ram_S": (None, [vp, _dp]),
            "ref_ram_started": (ci, [vp]),
            "ref_ram_accept_ratio": (cd, [vp]),
            "ref_ram_g0": (ci, [vp]),
            "ref_list_mean": (ci, [_dp, ci, ci, ci, _dp]),
            "ref_list_qtile": (ci, [_dp, ci, ci, ci, cd, _dp]),
            "ref_find_nan": (ci, [ci, _dp, _dp, ci, ci, ci, ci, _dp, pi]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    # ---- covariance_functions.{h,cpp}
    def transform(self, q, theta):
        """CovarianceParams(2, q, -1).transform(theta) -> dict(ai1, ai2, phi_i, thetamv, Dmat, covariance_model, npars, n_cbase)."""
        theta = _f(theta)
        ai1, ai2, phi = np.zeros(q), np.zeros(q), np.zeros(q)
        thetamv, D = np.zeros(3), np.zeros(max(1, q * q))
        dims = (C.c_int * 4)()
        _check(self._l.ref_transform(q, _d(theta), theta.size, _d(ai1), _d(ai2), _d(phi), _d(thetamv), _d(D), dims), "transform")
        p = dims[3]
        return dict(ai1=ai1, ai2=ai2, phi_i=phi, thetamv=thetamv[:dims[2]].copy(), Dmat=D[:p * p].reshape(p, p, order="F").copy(),
                    covariance_model=dims[0], npars=dims[1], n_cbase=dims[2])

    def vec_to_symmat(self, x):
        x = _f(x)
        p = C.c_int()
        out = np.zeros((x.size + 2) ** 2)
        _check(self._l.ref_vec_to_symmat(_d(x), x.size, _d(out), C.byref(p)), "vec_to_symmat")
        return out[:p.value ** 2].reshape(p.value, p.value, order="F").copy()

    def _cov(self, which, q, theta, coords, qv, ind1, ind2, same):
        theta, coords, qv, ind1, ind2 = _f(theta), _f(coords), _i(qv), _i(ind1), _i(ind2)
        assert coords.ndim == 2 and coords.shape[1] == 2 and qv.size == coords.shape[0]
        assert ind1.size == 0 or (ind1.min() >= 0 and ind1.max() < qv.size)
        assert ind2.size == 0 or (ind2.min() >= 0 and ind2.max() < qv.size)
        out = np.zeros((ind1.size, ind2.size), order="F")
        _check(self._l.ref_covariancef(which, q, _d(theta), theta.size, _d(coords), coords.shape[0], _l(qv), _l(ind1), ind1.size,
                                       _l(ind2), ind2.size, int(bool(same)), _d(out)), "Covariancef")
        return np.ascontiguousarray(out)

    def Covariancef(self, q, theta, coords, qv, ind1, ind2, same=False):
        return self._cov(0, q, theta, coords, qv, ind1, ind2, same)

    def mvCovAG20107(self, q, theta, coords, qv, ind1, ind2, same=False):
        return self._cov(1, q, theta, coords, qv, ind1, ind2, same)

    def CrossCovarianceAG10(self, coords1, mv1, coords2, mv2, ai1, ai2, phi_i, thetamv, Dmat):
        c1, c2, m1, m2 = _f(coords1), _f(coords2), _i(mv1), _i(mv2)
        ai1, ai2, phi_i, thetamv, D = _f(ai1), _f(ai2), _f(phi_i), _f(thetamv), _f(np.atleast_2d(Dmat))
        assert c1.shape == (m1.size, 2) and c2.shape == (m2.size, 2) and D.shape[0] == D.shape[1]
        assert ai1.size == ai2.size == phi_i.size and min(m1.min(), m2.min()) >= 1 and max(m1.max(), m2.max()) <= ai1.size
        out = np.zeros((m1.size, m2.size), order="F")
        _check(self._l.ref_cross_covariance_ag10(_d(c1), m1.size, _l(m1), _d(c2), m2.size, _l(m2), _d(ai1), _d(ai2), _d(phi_i),
                                                 ai1.size, _d(thetamv), thetamv.size, _d(D), D.shape[0], _d(out)),
               "CrossCovarianceAG10")
        return np.ascontiguousarray(out)

    # ---- mh_adapt.{h,cpp}
    def par_huvtransf_fwd(self, par, bounds):
        par, b, out = _f(par), _f(bounds), np.zeros(len(par))
        _check(self._l.ref_par_huvtransf_fwd(_d(par), par.size, _d(b), _d(out)), "par_huvtransf_fwd")
        return out

    def par_huvtransf_back(self, par, bounds):
        par, b, out = _f(par), _f(bounds), np.zeros(len(par))
        _check(self._l.ref_par_huvtransf_back(_d(par), par.size, _d(b), _d(out)), "par_huvtransf_back")
        return out

    def unif_bounds(self, par, bounds):
        """Returns (clamped copy of par, out_of_bounds flag)."""
        par, b, flag = _f(par), _f(bounds), C.c_int()
        _check(self._l.ref_unif_bounds(_d(par), par.size, _d(b), C.byref(flag)), "unif_bounds")
        return par, bool(flag.value)

    def calc_jacobian(self, new_param, param, bounds):
        a, b, bd, out = _f(new_param), _f(param), _f(bounds), C.c_double()
        _check(self._l.ref_calc_jacobian(_d(a), _d(b), b.size, _d(bd), C.byref(out)), "calc_jacobian")
        return out.value

    def do_I_accept(self, logaccept, u):
        """do_I_accept(logaccept) with R::runif(0, 1) returning u."""
        self._l.ref_runif_clear()
        u = _f([u])
        self._l.ref_runif_push(_d(u), 1)
        acc = C.c_int()
        _check(self._l.ref_do_I_accept(float(logaccept), C.byref(acc)), "do_I_accept")
        assert self._l.ref_runif_pending() == 0
        return bool(acc.value)

    def RAMAdapt(self, npars, metropolis_sd):
        return RefRAMAdapt(self._l, npars, metropolis_sd)

    # ---- list_mean.cpp, find_nan.cpp
    @staticmethod
    def _stack(x):
        mats = [np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in x]
        if np.asarray(x[0]).ndim == 1:
            mats = [m.T for m in mats]                       # a vector is one column
        r, c = mats[0].shape
        return np.concatenate([m.ravel(order="F") for m in mats]), len(mats), r, c

    def list_mean(self, x):
        flat, k, r, c = self._stack(x)
        out = np.zeros((r, c), order="F")
        _check(self._l.ref_list_mean(_d(flat), k, r, c, _d(out)), "list_mean")
        return np.ascontiguousarray(out).reshape(np.asarray(x[0]).shape)

    def list_qtile(self, x, q):
        flat, k, r, c = self._stack(x)
        out = np.zeros((r, c), order="F")
        _check(self._l.ref_list_qtile(_d(flat), k, r, c, float(q), _d(out)), "list_qtile")
        return np.ascontiguousarray(out).reshape(np.asarray(x[0]).shape)

    def _find(self, finite, infield, filtering):
        a, k, r, c = self._stack(infield)
        f, kf, rf, cf = self._stack(filtering)
        assert k == kf and r == rf
        out, rows = np.zeros(max(1, k * r * c)), (C.c_int * k)()
        _check(self._l.ref_find_nan(finite, _d(a), _d(f), k, r, c, cf, _d(out), rows), "find_nan")
        res, off = [], 0
        for i in range(k):
            res.append(out[off:off + rows[i] * c].reshape(rows[i], c, order="F").copy())
            off += rows[i] * c
        return res

    def find_not_nan(self, infield, filtering):
        return self._find(1, infield, filtering)

    def find_nan(self, infield, filtering):
        return self._find(0, infield, filtering)


def load():
    """The library, or None where oracle/_ref/libspamtree_ref.so does not exist."""
    if not _cached:
        _cached.append(RefLib(LIB_PATH) if os.path.exists(LIB_PATH) else None)
    return _cached[0]
