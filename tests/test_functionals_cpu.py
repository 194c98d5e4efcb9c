"""CPU-only: the Python front door of the linear functionals (model.functionals_csr, predict.areal_means, predict.contrasts,
fit.spamtree_mv_mcmc(new_points=dict(functionals=...))): the three accepted forms give one CSR, the helpers give hand-written
CSR, and every input error is a ValueError raised before any device call (no library is loaded here)."""
import numpy as np
import pytest

from spamtree_amd.model import functionals_csr
from spamtree_amd.predict import areal_means, contrasts


def same(a, b):
    return all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


HAND = (np.array([0, 2, 2, 5], dtype=np.int64), np.array([3, 0, 4, 1, 2], dtype=np.int64), np.array([0.5, -2.0, 1.0, 1e-3, 7.0]))


def test_three_forms_one_csr():
    assert same(functionals_csr(HAND, 5), HAND)
    assert same(functionals_csr(([0, 2, 2, 5], [3, 0, 4, 1, 2], [0.5, -2.0, 1.0, 1e-3, 7.0]), 5), HAND)
    pairs = [([3, 0], [0.5, -2.0]), ([], []), (np.array([4, 1, 2]), np.array([1.0, 1e-3, 7.0]))]
    assert same(functionals_csr(pairs, 5), HAND)
    assert same(functionals_csr(tuple(pairs), 5), HAND)          # a tuple of three pairs is the pair form, not CSR
    dense = np.zeros((3, 5))
    dense[0, 3], dense[0, 0] = 0.5, -2.0
    dense[2, 4], dense[2, 1], dense[2, 2] = 1.0, 1e-3, 7.0
    ptr, idx, wt = functionals_csr(dense, 5)      # zeros dropped; a dense row lists its points in ascending order
    assert np.array_equal(ptr, HAND[0])
    assert np.array_equal(idx, [0, 3, 1, 2, 4]) and np.array_equal(wt, [-2.0, 0.5, 1e-3, 7.0, 1.0])
    assert same(functionals_csr([], 5), (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)))
    assert functionals_csr(np.zeros((2, 0)), 0)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("bad,n,text", [
    ((np.array([1, 2]), np.array([0, 1]), np.array([1.0, 1.0])), 3, "ptr must start at 0"),
    ((np.array([0, 2, 1]), np.array([0, 1]), np.array([1.0, 1.0])), 3, "ptr must start at 0"),
    ((np.array([0, 3]), np.array([0, 1]), np.array([1.0, 1.0])), 3, "ptr must start at 0"),
    ((np.array([0, 2]), np.array([0, 1]), np.array([1.0])), 3, "ptr must start at 0"),
    ((np.array([0, 2]), np.array([0, 3]), np.array([1.0, 1.0])), 3, "indices must lie in 0..2"),
    ((np.array([0, 2]), np.array([-1, 2]), np.array([1.0, 1.0])), 3, "indices must lie in 0..2"),
    ((np.array([0, 2]), np.array([0, 1]), np.array([1.0, np.nan])), 3, "weights must be finite"),
    ((np.array([0, 2]), np.array([0, 1]), np.array([np.inf, 1.0])), 3, "weights must be finite"),
    ((np.array([0, 2, 4]), np.array([0, 1, 2, 2]), np.ones(4)), 3, "occurs twice"),
    ((np.array([0.0, 2.0]), np.array([0, 1]), np.ones(2)), 3, "must be integers"),
    ((np.array([[0, 2]]), np.array([0, 1]), np.ones(2)), 3, "one-dimensional"),
    (np.ones((2, 4)), 3, "dense array must be n_fun x n_new"),
    (np.ones(3), 3, "dense array must be n_fun x n_new"),
    (np.array([[1.0, np.nan, 0.0]]), 3, "weights must be finite"),
    ([([0, 1], [1.0])], 3, "2 indices and 1 weights"),
    ([([0.5], [1.0])], 3, "must be integers"),
    ([[0, 1, 2]], 3, "not an (indices, weights) pair"),
    ([([0, 0], [1.0, 1.0])], 3, "occurs twice"),
])
def test_input_errors_are_value_errors(bad, n, text):
    with pytest.raises(ValueError, match="functionals: ") as e:
        functionals_csr(bad, n)
    assert text in str(e.value), str(e.value)


def test_the_same_point_in_two_functionals_is_fine():
    ptr, idx, wt = functionals_csr([([1, 2], [1.0, 1.0]), ([2, 1], [1.0, -1.0])], 3)
    assert ptr.tolist() == [0, 2, 4] and idx.tolist() == [1, 2, 2, 1]


def test_areal_means_against_hand_written_csr():
    labels = np.array([2, -1, 0, 2, 0, 0, -7, 5])
    ptr, idx, wt = areal_means(labels)
    assert ptr.tolist() == [0, 3, 5, 6] and idx.tolist() == [2, 4, 5, 0, 3, 7]
    assert np.array_equal(wt, [1 / 3, 1 / 3, 1 / 3, 0.5, 0.5, 1.0])
    ptr, idx, wt = areal_means(labels, weights=np.array([1.0, 9.0, 2.0, 3.0, 2.0, 4.0, 9.0, 0.25]))
    assert ptr.tolist() == [0, 3, 5, 6] and idx.tolist() == [2, 4, 5, 0, 3, 7]
    assert np.array_equal(wt, [2.0 / 8.0, 2.0 / 8.0, 4.0 / 8.0, 1.0 / 4.0, 3.0 / 4.0, 1.0])
    assert same(functionals_csr(areal_means(labels), labels.size), areal_means(labels))
    assert areal_means(np.array([-1, -1]))[0].tolist() == [0]
    for bad in (dict(labels=np.array([0.5, 1.0])), dict(labels=np.zeros((2, 2), dtype=int)),
                dict(labels=np.array([0, 1]), weights=np.array([1.0])), dict(labels=np.array([0, 1]), weights=np.array([1.0, 0.0])),
                dict(labels=np.array([0, 1]), weights=np.array([1.0, np.nan]))):
        with pytest.raises(ValueError, match="areal_means"):
            areal_means(**bad)


def test_contrasts_against_hand_written_csr():
    ptr, idx, wt = contrasts([(4, 1), (0, 2), (1, 4)])
    assert ptr.tolist() == [0, 2, 4, 6] and idx.tolist() == [4, 1, 0, 2, 1, 4] and wt.tolist() == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0]
    assert same(functionals_csr(contrasts([(4, 1), (0, 2)]), 5), contrasts([(4, 1), (0, 2)]))
    assert contrasts([])[0].tolist() == [0]
    for bad in ([(1, 1)], [(0, -1)], [(0, 1, 2)], [(0.5, 1.0)]):
        with pytest.raises(ValueError, match="contrasts"):
            contrasts(bad)
    with pytest.raises(ValueError, match="indices must lie"):
        functionals_csr(contrasts([(0, 5)]), 5)


def test_the_fit_checks_functionals_before_any_device_call(monkeypatch):
    from spamtree_amd import _lib, fit, predict
    from tests.util import make_problem

    def no_device(*a, **k):
        raise AssertionError("the library was loaded before the inputs were checked")
    monkeypatch.setattr(_lib, "load", no_device)
    pts = dict(coords=np.zeros((4, 2)), mv=np.ones(4, dtype=np.int64), anchor=np.zeros(4, dtype=np.int64))
    assert fit._points_inputs(dict(pts, functionals=[([0, 3], [1.0, -1.0])]), 2, 1, ())[6][1].tolist() == [0, 3]
    assert fit._points_inputs(dict(pts, functionals=[]), 2, 1, ())[6] is None
    assert fit._points_inputs(pts, 2, 1, ())[6] is None
    for bad, text in (([([0, 4], [1.0, 1.0])], "indices must lie in 0..3"), ([([1, 1], [1.0, 1.0])], "occurs twice"),
                      (np.ones((1, 5)), "dense array"), ([([0], [np.inf])], "finite")):
        with pytest.raises(ValueError, match="new_points: functionals: ") as e:
            fit._points_inputs(dict(pts, functionals=bad), 2, 1, ())
        assert text in str(e.value)
    with pytest.raises(ValueError, match="unknown keys"):
        fit._points_inputs(dict(pts, functional=[]), 2, 1, ())
    pb = make_problem(side=8, q=1, seed=1)
    new = np.array([[0.2, 0.3], [0.6, 0.1]])
    with pytest.raises(ValueError, match="indices must lie in 0..1"):
        predict.fit_predict(pb, new, np.ones(2, dtype=np.int64), functionals=[([0, 2], [1.0, 1.0])], mcmc_keep=1, mcmc_burn=0)
    with pytest.raises(ValueError, match="indices must lie in 0..1"):
        predict.predict_new(pb, dict(w_mcmc=[]), new, np.ones(2, dtype=np.int64), functionals=[([0, 2], [1.0, 1.0])])
    with pytest.raises(ValueError, match="z=None and mode=0"):
        predict.predict_new(pb, dict(w_mcmc=[]), new, np.ones(2, dtype=np.int64), functionals=[([0, 1], [1.0, 1.0])], mode=1)
