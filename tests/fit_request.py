"""What tests/test_fit_request_cpu.py and tests/test_gpu_fit_request.py share: which fields of the whole-fit request (include/
spamtree_fit.h, stm_fit) each positional entry point sets, and the positional arguments that say what a request says."""
from spamtree_amd import _lib

# the positional entry points -> the parts of stm_fit they set beyond the run, in the order of their arguments
LEGACY = {
    "spamtree_mv_mcmc_c": (),
    "stm_mcmc_points": ("pts",),
    "stm_mcmc_points_joint": ("pts",),
    "stm_mcmc_functionals": ("pts", "fun"),
    "stm_mcmc_scored": ("pts", "fun", "scores"),
    "stm_mcmc_diagnosed": ("pts", "fun", "scores", "diag"),
    "stm_mcmc_excursions": ("pts", "fun", "scores", "diag", "exc"),
    "stm_mcmc_ranked": ("pts", "fun", "scores", "diag", "exc", "rk"),
    "stm_mcmc_chains": ("pts", "fun", "scores", "diag", "exc", "rk", "ch"),
    "stm_mcmc_criteria": ("criteria",),
    "stm_mcmc_loo": ("criteria", "loo"),
}
POINTS_FAMILY = ("pts", "fun", "scores", "diag", "exc", "rk", "ch")


def positional(symbol, req):
    """The arguments of ``symbol`` for the request ``req`` (an _lib.StmFit that sets no part the symbol cannot express): the run's
    fields, the point set's (a NULL pts: the empty set of no pointer) and one pointer per further part."""
    parts = LEGACY[symbol]
    assert not any(getattr(req, name) for name, _ in _lib.StmFit._fields_[1:] if name not in parts), symbol
    args = [getattr(req.run, name) for name, _ in _lib.StmRun._fields_]
    if "pts" in parts:
        pts = req.pts.contents if req.pts else _lib.StmNewPoints()
        skip = _lib.JOINT_ONLY if symbol == "stm_mcmc_points" else ()
        assert not any(getattr(pts, name) for name in skip), symbol
        args += [getattr(pts, name) for name, _ in _lib.StmNewPoints._fields_ if name not in skip]
    return args + [getattr(req, name) for name in parts if name != "pts"]
