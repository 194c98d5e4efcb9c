"""Worker for the multi-process tests (spawned with torch.multiprocessing; gloo backend, 127.0.0.1 rendezvous)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _init(rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def plan_worker(rank, world, port, case, out_dir):
    """CPU only: the library's pure-host ownership plan + the sum-with-zeros exchange, with the oracle as compute."""
    import torch
    dist = _init(rank, world, port)
    from spamtree_amd import _lib
    from spamtree_amd.model import _lists_to_csr, _i64, _f64, _dp, _ip
    from spamtree_amd.sharded import shard_plan
    from tests.util import make_problem, oracle_model
    pb = make_problem(**case)
    y = _f64(pb["y"]); X = np.asfortranarray(pb["X"]); co = np.asfortranarray(pb["coords"]); mv = _i64(pb["mv_id"])
    ip, ii = _lists_to_csr(pb["indexing"]); pp, pi = _lists_to_csr(pb["parents"]); cp, ci = _lists_to_csr(pb["children"])
    keep = [_i64(pb["res_is_ref"]), _i64(pb["block_names"]), _i64(pb["block_groups"]), ip, ii, pp, pi, cp, ci]
    st = _lib.StProblem(pb["n"], 2, pb["q"], pb["p"], int(keep[0].size), int(keep[1].size), _dp(y), _dp(X), _dp(co), _ip(mv),
                        *[_ip(a) for a in keep])
    owner, cut = shard_plan(st, world, limited_tree=bool(case.get("limited_tree", False)))
    nb = owner.size
    levels = np.unique(pb["block_groups"])
    lev_of = np.searchsorted(levels, pb["block_groups"])
    # ---- plan invariants
    assert np.all(owner[lev_of < cut] == -1), "levels above the cut must be replicated"
    obs_blocks = np.array([np.isfinite(pb["y"][ix]).any() for ix in pb["indexing"]])
    below = (lev_of >= cut)
    assert np.all(owner[below] >= 0) and np.all(owner[below] < world)
    for u in range(nb):                                  # a block below the cut inherits its cut-level ancestor's rank
        if lev_of[u] > cut:
            a = u                                        # walk the direct parents up to the cut level (full lists: the last entry;
            while lev_of[a] > cut:                       # make_edges_limited's lists: the only one)
                a = pb["parents"][a][-1]
            assert lev_of[a] == cut and owner[a] == owner[u]
    if cut < levels.size:
        assert len(set(owner[below].tolist())) == world, "every rank owns at least one subtree"
    # ---- exchange: every rank masks a full oracle result to what it owns; the all-reduce restores it bit for bit
    rng = np.random.default_rng(9)
    om = oracle_model(pb, w=rng.standard_normal(pb["n"]), tausq=0.2)
    assert om.get_loglik_comps_w(om.param_data)
    om.gibbs_sample_w(rng.standard_normal(pb["n"]))
    mine_blk = (owner == rank) | ((owner == -1) & (rank == 0))
    comps = np.concatenate([np.where(mine_blk, om.param_data.logdetCi_comps, 0.0), np.where(mine_blk, om.param_data.loglik_w_comps, 0.0)])
    rowmask = np.zeros(pb["n"], dtype=bool)
    for u in range(nb):
        if mine_blk[u]:
            rowmask[pb["indexing"][u]] = True
    wbuf = np.where(rowmask, om.w, 0.0)
    tc, tw = torch.from_numpy(comps.copy()), torch.from_numpy(wbuf.copy())
    dist.all_reduce(tc); dist.all_reduce(tw)
    full = np.concatenate([om.param_data.logdetCi_comps, om.param_data.loglik_w_comps])
    assert np.array_equal(tc.numpy(), full) and np.array_equal(tw.numpy(), om.w)
    cnt = torch.from_numpy(rowmask.astype(np.int64)); dist.all_reduce(cnt)
    assert np.all(cnt.numpy() == 1), "every row is contributed by exactly one rank"
    np.save(os.path.join(out_dir, f"ok_{rank}.npy"), np.array([cut]))
    dist.destroy_process_group()


FAILURE_CASE = dict(side=40, q=1, seed=21, missing=0.05)      # the two-rank failure case of tests/test_gpu_sharded.py


def failure_problem(case):
    """make_problem(**case) with rows of its deepest level relabelled as a further outcome (tests/util.level_failure_problem),
    all of them inside subtrees that ONE rank -- the second -- of the two-rank plan owns.  Returns (pb, relabelled problem,
    its failing inputs, the level, the plan's owners)."""
    from spamtree_amd.sharded import shard_plan
    from tests.util import level_failure_problem, make_problem, problem_arrays, st_problem_struct
    pb = make_problem(**case)
    arrays = problem_arrays(pb)
    owner, cut = shard_plan(st_problem_struct(arrays), 2)
    labels = np.unique(pb["block_groups"])
    observed = [u for u, ix in enumerate(pb["indexing"]) if np.isfinite(pb["y"][ix]).any()]
    level = int(np.searchsorted(labels, max(pb["block_groups"][u] for u in observed)))
    assert level >= cut
    blocks = [u for u in observed if pb["block_groups"][u] == labels[level] and owner[u] == 1]
    fp, f = level_failure_problem(pb, level, blocks=blocks)
    rng = np.random.default_rng(7)
    f.update(w=rng.standard_normal(pb["n"]), zs=[rng.standard_normal(pb["n"]) for _ in range(3)], theta2=fp["theta"] * 1.03)
    return pb, fp, f, level, owner


def failure_problem_on_oracle(case):
    """failure_problem(case) checked on the oracle, no GPU involved: every relabelled row lies in a subtree of the second
    rank, phase A at theta_bad fails at that level with errtype 3 (shallower levels succeed), the sweep with the bad
    tausq^-1 fails there only with 11.  Returns failure_problem's tuple and the oracle's w after the sweep with zs[2] from
    the restored state."""
    from tests.util import oracle_model, oracle_phase_a_failure, oracle_sweep_failing_levels
    pb, fp, f, level, owner = failure_problem(case)
    block_of = np.empty(pb["n"], dtype=np.int64)
    for u, ix in enumerate(pb["indexing"]):
        block_of[ix] = u
    assert f["rows"].size >= 4 and np.all(owner[block_of[f["rows"]]] == 1) and np.any(owner == 0)
    om = oracle_model(fp, theta=fp["theta"], w=f["w"], beta=np.array([0.3, -0.2, 0.1]), tausq=1.0 / f["tausq_inv_ok"])
    assert om.get_loglik_comps_w(om.param_data)
    om.theta_update(om.alter_data, f["theta_bad"])
    assert oracle_phase_a_failure(om, om.alter_data) == (3, level)
    om.gibbs_sample_w(f["zs"][0])

    def set_tausq_inv(t):
        om.tausq_inv = t.copy()
        om.tausq_inv_long = om.tausq_inv[om.mv_id - 1].astype(np.float64)

    set_tausq_inv(f["tausq_inv_bad"])
    with np.errstate(all="ignore"):
        try:
            om.gibbs_sample_w(f["zs"][1])
        except RuntimeError:
            pass
    assert om.last_sample_errtype == 11 and oracle_sweep_failing_levels(om) == [level]
    set_tausq_inv(f["tausq_inv_ok"])
    om.w = f["w"].copy()
    om.gibbs_sample_w(f["zs"][2])
    return (pb, fp, f, level, owner), om.w.copy(), om.na_ix_all


def _failure_case(rank, world, dist, case, out_dir):
    """A phase-A and a sweep failure that only one rank's kernels see: the codes every rank reports (phase A; the sweep with
    w exchanged by all-gather, by all-reduce and in the fused form), and the state every rank has afterwards."""
    from spamtree_amd.model import SpamTreeError, _dp, _f64
    from spamtree_amd.sharded import ShardedSpamTreeMV
    _, fp, f, level, _ = failure_problem(case)
    m = ShardedSpamTreeMV(fp["y"], fp["X"], fp["Z"], fp["coords"], fp["mv_id"], fp["blocking"], fp["gix_block"],
                          fp["res_is_ref"], fp["parents"], fp["children"], False, fp["block_names"], fp["block_groups"],
                          fp["indexing"], f["w"], np.array([0.3, -0.2, 0.1]), fp["theta"], 1.0, device=0,
                          dist=dist if world > 1 else None)

    def set_tausq_inv(t):
        m.tausq_inv = _f64(t).copy()
        m._check(m.lib.st_set_tausq_inv(m.h, _dp(m.tausq_inv)))

    set_tausq_inv(f["tausq_inv_ok"])
    res = {}
    assert m.get_loglik_comps_w(0)
    res["ll_A"] = m.loglik_w[0]
    m.theta_update(1, f["theta_bad"])
    assert m.get_loglik_comps_w(1) is False
    res["a_code"] = m.last_errtype
    m.theta_update(1, f["theta2"])
    assert m.get_loglik_comps_w(1)
    res["ll_A2"] = m.loglik_w[1]
    m.deal_with_w(f["zs"][0])
    res["w_0"] = m.get_w().copy()
    for form in ("gather", "allreduce", "fused"):
        m.use_allreduce_w = form == "allreduce"
        set_tausq_inv(f["tausq_inv_bad"])
        m.set_w(f["w"])
        try:
            if form == "fused":
                m.deal_with_w_loglik(0, f["zs"][1])
            else:
                m.deal_with_w(f["zs"][1])
            res[f"s_code_{form}"] = -1
        except SpamTreeError:
            res[f"s_code_{form}"] = m.last_sample_errtype
        set_tausq_inv(f["tausq_inv_ok"])
        m.set_w(f["w"])
        res[f"ll_{form}"] = m.deal_with_w_loglik(0, f["zs"][2])
        res[f"w_{form}"] = m.get_w().copy()
    m.accept_make_change()
    m.deal_with_w(f["zs"][1])
    res["w_accepted"] = m.get_w().copy()
    np.savez(os.path.join(out_dir, f"fail_{world}_{rank}.npz"), level=level, **res)
    m.close()


def gpu_worker(rank, world, port, side, q, out_dir, steps, limited=False, failure=None):
    """Needs a GPU: `world` processes share device 0 and one problem; results go to out_dir for the parent to compare.
    failure: the make_problem keywords of a failure case (_failure_case), run in place of the protocol below."""
    dist = _init(rank, world, port)
    if failure is not None:
        _failure_case(rank, world, dist, failure, out_dir)
        dist.destroy_process_group()
        return
    from spamtree_amd.sharded import ShardedSpamTreeMV
    from spamtree_amd.synthetic import make_workload
    wl = make_workload(side, q=q, limited_tree=limited)
    m = ShardedSpamTreeMV(wl["y"], wl["X"], wl["Z"], wl["coords"], wl["mv_id"], wl["blocking"], wl["gix_block"],
                          wl["res_is_ref"], wl["parents"], wl["children"], bool(limited), wl["block_names"], wl["block_groups"],
                          wl["indexing"], np.zeros(wl["n"]), np.array([-0.5, 0.2, 0.4]), wl["theta"], 1.0 / 0.15,
                          device=0, dist=dist if world > 1 else None, allreduce_w=(world == 3))   # both forms of the w exchange
    rng = np.random.default_rng(3)
    m.set_w(rng.standard_normal(wl["n"]))
    res = {}
    assert m.get_loglik_comps_w(0)
    res["ll_A"] = m.loglik_w[0]
    for it in range(steps):
        if it % 2 == 1 and world > 1:             # the fused order: phase C before the exchange of w, one exchange for both
            res[f"ll_C{it}"] = m.deal_with_w_loglik(0, None, seed=5, it=it)
        else:
            m.deal_with_w(None, seed=5, it=it)
            res[f"ll_C{it}"] = m.get_loglik_w(0)
    th2 = wl["theta"] * 1.03
    m.theta_update(1, th2)
    assert m.get_loglik_comps_w(1)
    res["ll_A2"] = m.loglik_w[1]
    res["err"] = 0.0
    if q == 1:                                   # negative sigma^2: every rank must agree on the failure code
        bad = wl["theta"].copy(); bad[0] = -1.0
        m.theta_update(1, bad)
        assert m.get_loglik_comps_w(1) is False
        res["err"] = float(m.last_errtype)
    xty, ssq = m.stats()
    info = m.shard_info() if world > 1 else {}
    kernels = np.array([{"generic_lds": 0, "generic_scratch": 1, "k_factor_mfma": 2, "k_factor_quad": 3, "k_factor_bigmfma": 4,
                         "k_factor_wide": 5, "k_factor_lchain": 6, "k_factor_lchain+ref_finish": 7}[L["kernel"]] for L in m.level_info()])
    np.savez(os.path.join(out_dir, f"res_{world}_{rank}.npz"), w=m.get_w(), xty=xty, ssq=ssq,
             owned_rows=info.get("owned_rows", wl["n"]), kernels=kernels, **res)
    m.close()
    dist.destroy_process_group()
