"""GPU: the elementary functions every covariance entry goes through (csrc/st_device.hpp), at ulp level.

st_probe_math evaluates cov_sqrt, cov_exp and cov_exp_tab through the same inlined helpers the kernels use.  The claims of
their comments are checked as written:
  - cov_sqrt is the correctly rounded square root of max(a, 1e-270): bitwise equal to np.sqrt over every binade from 2^-996 to
    2^996 (edge mantissas and 64 random ones each), the squared grid distances of config #3, random squared distances, 0,
    subnormals and the clamp;
  - cov_exp / cov_exp_tab have relative error < 3e-16 on normal results and at most one subnormal ulp below 2^-1022, over
    [-1500, 0], the rounding switches of both reductions, the subnormal band, and the clamped tail (exactly +0).
The yardstick is exp in 80-bit long double, itself checked against mpmath at 50 digits on a sample of every input set.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
SQRT, EXP, EXP_TAB = 0, 1, 2
TINY = 2.0 ** -1074
REL_EXP = 3e-16          # the documented claim of cov_exp / cov_exp_tab
SQRT_CLAMP = 1e-270      # cov_sqrt's lower clamp: coincident points give 1e-135
LN2 = LD("0.693147180559945309417232121458176568")


def probe(fn, x):
    from spamtree_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(x.size, np.nan)
    rc = _lib.load().st_probe_math(fn, x.ctypes.data_as(_lib.c_dp), x.size, 0, out.ctypes.data_as(_lib.c_dp))
    assert rc == 0, rc
    return out


def around(centres, k=4):
    """Every double within k ulps of each centre."""
    c = np.asarray(centres, dtype=np.float64)
    pts = [c]
    lo, hi = c.copy(), c.copy()
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        pts += [lo, hi]
    return np.concatenate(pts)


def exp_ref(x):
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(x, dtype=LD))


def check_ref_against_mpmath(x, n=400, seed=0):
    """The long-double reference agrees with mpmath to far below the tolerance on a sample of x."""
    import mpmath as mp
    rng = np.random.default_rng(seed)
    xs = x if x.size <= n else rng.choice(x, n, replace=False)
    ref = exp_ref(xs)
    with mp.workdps(50):
        for xi, ri in zip(xs, ref):
            e = mp.exp(mp.mpf(float(xi)))
            if e == 0:
                continue
            assert abs(mp.mpf(str(ri)) - e) <= mp.mpf("1e-18") * e, xi


def check_exp(fn, x, what):
    x = np.asarray(x, dtype=np.float64)
    got = probe(fn, x)
    ref = exp_ref(x)
    normal = ref >= LD(2.0 ** -1022)
    rel = np.abs((got[normal].astype(LD) - ref[normal]) / ref[normal])
    worst = int(np.argmax(rel)) if rel.size else 0
    assert rel.size == 0 or rel.max() < REL_EXP, (what, float(rel.max()), float(x[normal][worst]))
    # subnormal and underflowing results: at most one ulp (2^-1074) from the correctly rounded value
    sub = ~normal
    err = np.abs(got[sub] - ref[sub].astype(np.float64))
    assert err.size == 0 or err.max() <= TINY, (what, float(err.max()), float(x[sub][int(np.argmax(err))]))
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), what
    return float(rel.max()) if rel.size else 0.0


def exp_inputs():
    rng = np.random.default_rng(20)
    uniform = -rng.uniform(0.0, 1500.0, 2 ** 20)
    k = np.arange(-2165, 0)
    switch = around(((k + 0.5) * LN2).astype(np.float64))
    kt = np.arange(-138500, 0)
    switch_tab = around(((kt + 0.5) * LN2 / 64).astype(np.float64))
    subnormal = np.concatenate([np.linspace(-745.2, -708.3, 2 ** 16), -rng.uniform(708.3, 745.2, 2 ** 16)])
    return dict(uniform=uniform, switch=switch, switch_tab=switch_tab, subnormal=subnormal)


@pytest.mark.parametrize("fn", [EXP, EXP_TAB], ids=["cov_exp", "cov_exp_tab"])
def test_cov_exp_relative_error_below_documented_bound(fn):
    worst = {}
    for what, x in exp_inputs().items():
        x = x[(x <= 0.0) & (x >= -1500.0)]
        check_ref_against_mpmath(x, seed=len(what))
        worst[what] = check_exp(fn, x, what)
    print("max relative error", worst)


@pytest.mark.parametrize("fn", [EXP, EXP_TAB], ids=["cov_exp", "cov_exp_tab"])
def test_cov_exp_edges(fn):
    ones = probe(fn, np.array([-0.0, 0.0, -TINY, -1e-300, -1e-200, -2.0 ** -60]))
    assert np.all(ones == 1.0), ones
    zeros = probe(fn, np.array([-1500.0, np.nextafter(-1500.0, -np.inf), -1e4, -1e300, -np.finfo(np.float64).max, -np.inf]))
    assert np.all(zeros == 0.0) and not np.any(np.signbit(zeros)), zeros
    # NaN: the argument is clamped with fmax(x, -1500) first, which returns -1500 for a NaN x, so the covariance of a NaN
    # distance is 0, not NaN (libm: NaN).  st_create refuses non-finite coordinates for that reason (test below).
    nan = probe(fn, np.array([np.nan, -np.nan]))
    assert np.all(nan == 0.0), nan


def sqrt_inputs():
    rng = np.random.default_rng(21)
    e = np.arange(-996, 996)
    mant = np.concatenate([np.array([1.0, 1.0 + 2.0 ** -52, 1.5, 2.0 - 2.0 ** -52]), 1.0 + rng.uniform(size=64)])
    binades = np.ldexp(mant[None, :], e[:, None]).ravel()
    g = np.linspace(0.0, 1.0, 1000)          # config #3: the 1000 x 1000 grid on [0, 1]^2
    i1, i2, j1, j2 = (rng.integers(0, 1000, 2 ** 20) for _ in range(4))
    dx, dy = g[i1] - g[i2], g[j1] - g[j2]
    grid = dx * dx + dy * dy
    ii, jj = np.meshgrid(np.arange(1000), np.arange(1000), indexing="ij")
    dx0, dy0 = g[ii.ravel()] - g[0], g[jj.ravel()] - g[0]
    grid0 = dx0 * dx0 + dy0 * dy0
    a, b = rng.uniform(size=(2 ** 18, 2)), rng.uniform(size=(2 ** 18, 2))
    d = a - b
    rand = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    near = rng.uniform(size=(2 ** 16, 2)) * 1e-7          # near-coincident points
    rand_near = near[:, 0] ** 2 + near[:, 1] ** 2
    small = np.concatenate([[0.0, -0.0, TINY, 2.0 ** -1022, np.nextafter(2.0 ** -1022, 0.0), 1e-310],
                            around([1e-300, 1e-270], 1), around([1e-271, 1e-269, 1e-250], 2)])
    return dict(binades=binades, grid=grid, grid_origin=grid0, random=rand, random_near=rand_near, small=small)


def test_cov_sqrt_is_correctly_rounded():
    for what, a in sqrt_inputs().items():
        got = probe(SQRT, a)
        want = np.sqrt(np.maximum(a, SQRT_CLAMP))
        bad = got != want
        assert not bad.any(), (what, int(bad.sum()), a[bad][:4], got[bad][:4], want[bad][:4])
    nan = probe(SQRT, np.array([np.nan]))
    assert nan[0] == np.sqrt(SQRT_CLAMP), nan       # fmax(NaN, clamp) = clamp, as for cov_exp


def test_probe_math_refuses_bad_arguments():
    from spamtree_amd import _lib
    lib = _lib.load()
    x = np.zeros(4)
    out = np.zeros(4)
    assert lib.st_probe_math(3, x.ctypes.data_as(_lib.c_dp), 4, 0, out.ctypes.data_as(_lib.c_dp)) < 0
    assert lib.st_probe_math(0, None, 4, 0, out.ctypes.data_as(_lib.c_dp)) < 0
    assert lib.st_probe_math(0, x.ctypes.data_as(_lib.c_dp), -1, 0, out.ctypes.data_as(_lib.c_dp)) < 0
    assert lib.st_probe_math(0, None, 0, 0, None) == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_create_refuses_non_finite_coordinates(bad):
    from spamtree_amd.model import SpamTreeError, SpamTreeMV
    from tests.util import make_problem
    pb = make_problem(side=8, q=1, seed=1)

    def create(coords):
        return SpamTreeMV(pb["y"], pb["X"], pb["Z"], coords, pb["mv_id"], pb["blocking"], pb["gix_block"],
                          pb["res_is_ref"], pb["parents"], pb["children"], False, pb["block_names"], pb["block_groups"],
                          pb["indexing"], np.zeros(pb["n"]), np.zeros(pb["p"]), pb["theta"], 10.0)

    coords = pb["coords"].copy()
    coords[17, 1] = bad
    with pytest.raises(SpamTreeError, match="coordinates must be finite") as e:
        create(coords)
    assert "st_create failed (-1)" in str(e.value)              # ST_ERR_USAGE
    hm = create(pb["coords"])                                   # the library is still usable
    assert hm.get_loglik_comps_w(0) and np.isfinite(hm.loglik_w[0])
    hm.close()
