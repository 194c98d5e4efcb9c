"""Everything the host-side layout of st_create decides, as text, so that two builds of the library can be diffed:

    SPAMTREE_LIB=<one build> python profiles/micro/layout_dump.py > a.txt
    SPAMTREE_LIB=<other build> python profiles/micro/layout_dump.py > b.txt

Problems: every row of ROUTES and WIDE_ROUTES of tests/test_gpu_routes.py (with the row's switches) and the bench default
(the 1000^2 grid).  Per problem, on one GPU: st_level_info, st_shard_info, a hash of st_block_dims over all blocks,
st_algorithmic_bytes, then st_route_info after phase A on both slots, after a sweep that rebuilds the Gram parts, after one
that reads them from the cache and after st_predict (rows with NA blocks), the log-densities and a hash of w (so a layout
that differs only in a place the routes do not show still shows), and st_points_info for a fixed point set.  Two rows are
also created as rank 1 of 2: their static figures only (the sharded protocol needs both ranks).  Needs a GPU."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from spamtree_amd.model import SpamTreeMV                                              # noqa: E402
from spamtree_amd.predict import locate                                                # noqa: E402
from spamtree_amd.synthetic import make_workload                                       # noqa: E402
from tests.test_gpu_routes import ROUTES, WIDE_ROUTES, build_problem, inputs          # noqa: E402

SHARDED = ("grid_leaf32_pred32", "wide4_default_pred")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def model(pb, inp, limited, force_generic=False, rank=0, world=1):
    return SpamTreeMV(pb["y"], pb["X"], pb["Z"], pb["coords"], pb["mv_id"], pb["blocking"], pb["gix_block"], pb["res_is_ref"],
                      pb["parents"], pb["children"], limited, pb["block_names"], pb["block_groups"], pb["indexing"], inp["w"],
                      inp["beta"], inp["theta"], 1.0 / inp["tausq"], force_generic=force_generic, rank=rank, world=world)


def static_info(tag, hm):
    print(tag, "level_info", hm.level_info())
    r, w, c, ob, orow = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    hm._check(hm.lib.st_shard_info(hm.h, C.byref(r), C.byref(w), C.byref(c), C.byref(ob), C.byref(orow)))
    print(tag, "shard_info", r.value, w.value, c.value, ob.value, orow.value)
    dims = np.zeros((hm.n_blocks, 4), dtype=np.int64)
    for u in range(hm.n_blocks):
        m, P, isref, nobs = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        hm._check(hm.lib.st_block_dims(hm.h, u, C.byref(m), C.byref(P), C.byref(isref), C.byref(nobs)))
        dims[u] = (m.value, P.value, isref.value, nobs.value)
    print(tag, "block_dims", hm.n_blocks, sha(dims))
    print(tag, "algorithmic_bytes", hm.algorithmic_bytes())


def dump(tag, pb, inp, limited=False, force_generic=False, topo=None):
    hm = model(pb, inp, limited, force_generic)
    static_info(tag, hm)
    assert hm.get_loglik_comps_w(0)
    hm.theta_update(1, inp["theta2"])
    assert hm.get_loglik_comps_w(1)
    print(tag, "routes A", hm.route_info(), "loglik", [float(v).hex() for v in hm.loglik_w])
    for what, z in (("rebuild", inp["zs"][0]), ("cached", inp["zs"][1])):
        hm.deal_with_w(z)
        print(tag, "routes", what, hm.route_info(), "loglik", float(hm.get_loglik_w(0)).hex(), "w", sha(hm.get_w()))
    if np.any(~np.isfinite(pb["y"])):
        hm.predict(True)
        print(tag, "routes predict", hm.route_info(), "w", sha(hm.get_w()))
    if topo is not None and not limited:
        rng = np.random.default_rng(5)
        n_new = 300
        co = rng.uniform(0.02, 0.98, size=(n_new, 2)) * np.ptp(pb["coords"], axis=0) + pb["coords"].min(axis=0)
        mv = rng.integers(1, pb["q"] + 1, size=n_new)
        hm.set_points(co, mv, locate(topo, co, mv), X=rng.standard_normal((n_new, pb["p"])))
        out = hm.predict_points(mode=0, z=rng.standard_normal(n_new))
        print(tag, "points_info", hm.points_info(), "w", sha(out["w"]), "var", sha(out["var"]))
    hm.close()


def main():
    only = set(sys.argv[1].split(",")) if len(sys.argv) > 1 else None
    for row in ROUTES + WIDE_ROUTES:
        if only and row["id"] not in only:
            continue
        for k in [k for k in os.environ if k.startswith("SPAMTREE_") and k != "SPAMTREE_LIB"]:
            del os.environ[k]
        os.environ.update(row["env"])
        pb = build_problem(row)
        inp = inputs(pb)
        limited = bool(pb.get("limited_tree", False))
        dump(row["id"], pb, inp, limited, bool(row.get("force_generic", False)), topo=pb["topo"])
        if row["id"] in SHARDED:
            hm = model(pb, inp, limited, rank=1, world=2)
            static_info(row["id"] + "@rank1of2", hm)
            hm.close()
        sys.stdout.flush()
    if only and "bench" not in only:
        return
    for k in [k for k in os.environ if k.startswith("SPAMTREE_") and k != "SPAMTREE_LIB"]:
        del os.environ[k]
    wl = make_workload(1000)
    rng = np.random.default_rng(7)
    inp = dict(w=rng.standard_normal(wl["n"]), beta=np.array([0.3, -0.2, 0.1]), tausq=0.2, theta=wl["theta"],
               theta2=wl["theta"] * 1.03, zs=[rng.standard_normal(wl["n"]) for _ in range(2)])
    wl.setdefault("q", 1)
    wl.setdefault("p", 3)
    dump("bench_default", wl, inp)


if __name__ == "__main__":
    main()
