"""CPU-only: the prior sweep st_simulate runs, restated in NumPy from the oracle's per-block factors, has the covariance of
the DAG model (the inverse of its dense precision); the front door rejects bad inputs before the library loads."""
import numpy as np
import pytest

from tests.prior_sweep import prior_sweep
from tests.test_oracle_identities import dense_precision
from tests.util import make_problem, oracle_model


@pytest.mark.parametrize("q,limited", [(1, False), (2, False), (1, True), (2, True)])
def test_restated_sweep_has_the_dag_covariance(q, limited):
    pb = make_problem(side=20, q=q, seed=3, limited_tree=limited)
    om = oracle_model(pb)
    assert om.get_loglik_comps_w(om.param_data)
    A = prior_sweep(om, np.eye(pb["n"]))
    Q, _ = dense_precision(pb, pb["theta"])
    C = np.linalg.inv(Q)
    err = np.abs(A @ A.T - C).max() / np.abs(C).max()
    assert err <= 1e-10, err


def _coords(n=50):
    return np.random.default_rng(0).uniform(size=(n, 2))


@pytest.mark.parametrize("kw", [
    dict(coords=np.zeros((5, 3))),
    dict(coords=np.array([[0.1, np.nan], [0.2, 0.3]])),
    dict(theta=[2.3, 1.0, 1.0]),
    dict(theta=[2.3, 1.0, np.inf, 6.0]),
    dict(mv_id=np.r_[np.ones(25), 3 * np.ones(25)]),
    dict(mv_id=np.zeros(50)),
    dict(mv_id=np.ones(49)),
    dict(X=np.ones((49, 2)), beta=[1.0, 2.0]),
    dict(X=np.ones((50, 2)), beta=[1.0, 2.0, 3.0]),
    dict(X=np.full((50, 1), np.nan), beta=[1.0]),
    dict(beta=[1.0]),
    dict(tausq=-1.0),
    dict(tausq=[0.1, 0.2]),
    dict(n_draws=0),
])
def test_simulate_rejects_bad_inputs(kw, monkeypatch):
    from spamtree_amd import _lib, simulate

    def no_load():
        raise AssertionError("the library was loaded before the inputs were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    args = dict(coords=_coords(), theta=[2.3, 1.0, 1.0, 6.0])
    args.update(kw)
    with pytest.raises(ValueError):
        simulate.simulate(**args)


def test_as_workload_rejects_bad_inputs():
    from spamtree_amd import simulate
    sim = dict(w=np.zeros((10, 2)), y=np.zeros((10, 2)), coords=_coords(10), mv_id=np.ones(10, dtype=np.int64),
               theta=np.array([2.3, 1.0, 1.0, 6.0]), beta=np.zeros((1, 1)), X=None)
    with pytest.raises(ValueError):
        simulate.as_workload(sim, draw=2)
    with pytest.raises(ValueError):
        simulate.as_workload(sim, missing=[1.0])
    with pytest.raises(ValueError):
        simulate.as_workload(sim, missing=[0.1, 0.2])
    with pytest.raises(ValueError):
        simulate.as_workload({"y": 1})
