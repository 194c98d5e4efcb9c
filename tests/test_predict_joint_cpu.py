"""CPU-only: the host side of joint new-point prediction -- the site labels, one anchor per joint group, and the checks that
raise before any device call."""
import numpy as np
import pytest

from tests.util import make_problem


def test_group_sites_labels_identical_coordinates_by_first_appearance():
    from spamtree_amd.predict import group_sites
    c = np.array([[0.5, 0.25], [0.1, 0.9], [0.5, 0.25], [0.3, 0.3], [0.1, 0.9], [0.5, 0.25 + 1e-12]])
    assert np.array_equal(group_sites(c), [0, 1, 0, 2, 1, 3])
    assert group_sites(np.zeros((0, 2))).size == 0
    assert group_sites(c).dtype == np.int64


def test_locate_gives_a_joint_group_the_anchor_of_its_first_member():
    from spamtree_amd.predict import locate
    pb = make_problem(side=20, q=2, seed=3, missing=0.1)
    rng = np.random.default_rng(4)
    pts = rng.uniform(size=(200, 2))
    mv = rng.integers(1, 3, size=200)
    plain = locate(pb["topo"], pts, mv)
    labels = rng.integers(0, 40, size=200) * 7 - 50
    joint = locate(pb["topo"], pts, mv, joint=labels)
    assert np.unique(plain).size > 1 and not np.array_equal(plain, joint)
    for lab in np.unique(labels):
        m = np.nonzero(labels == lab)[0]
        assert np.all(joint[m] == plain[m[0]]), lab
    assert np.array_equal(locate(pb["topo"], pts, mv, joint=np.arange(200)), plain)


def test_locate_gives_a_site_of_all_six_outcomes_one_anchor():
    """q = 6: 30 sites, each asked for with all six outcomes (interleaved in the caller's order): group_sites labels every
    site's six points alike, and locate(joint=) gives the six the anchor of the first, whichever outcome that is."""
    from spamtree_amd.predict import group_sites, locate
    pb = make_problem(side=10, q=6, seed=3, missing=[0.05, 0.1, 0.15, 0.2, 0.3, 0.4])
    rng = np.random.default_rng(4)
    perm = rng.permutation(180)
    pts = np.tile(rng.uniform(size=(30, 2)), (6, 1))[perm]
    mv = np.repeat(np.arange(1, 7), 30)[perm]
    labels = group_sites(pts)
    assert np.unique(labels).size == 30 and np.all(np.bincount(labels) == 6)
    plain = locate(pb["topo"], pts, mv)
    joint = locate(pb["topo"], pts, mv, joint=labels)
    for lab in range(30):
        m = np.nonzero(labels == lab)[0]
        assert sorted(mv[m]) == [1, 2, 3, 4, 5, 6] and np.all(joint[m] == plain[m[0]]), lab


def test_bad_joint_labels_raise_before_any_device_call():
    from spamtree_amd import fit
    from spamtree_amd.model import joint_labels
    from spamtree_amd.predict import locate
    pb = make_problem(side=20, q=2, seed=3, missing=0.1)
    pts = np.random.default_rng(4).uniform(size=(40, 2))
    mv = np.ones(40, dtype=np.int64)
    for bad, what in [(np.zeros(39, dtype=np.int64), "one label per point"), (np.zeros((40, 1), dtype=np.int64), "one label per point"),
                      (np.arange(40) / 2.0, "integers"), (np.arange(40) // 17, "at most 16")]:
        with pytest.raises(ValueError, match=what):
            joint_labels(bad, 40)
        with pytest.raises(ValueError, match=what):
            locate(pb["topo"], pts, mv, joint=bad)
        with pytest.raises(ValueError, match=what):
            fit._points_inputs(dict(coords=pts, mv=mv, anchor=np.zeros(40, dtype=np.int64), joint=bad), pb["p"], 2, ())
    assert np.array_equal(joint_labels(np.arange(40) // 16, 40), np.arange(40) // 16)
    with pytest.raises(ValueError, match="unknown keys"):
        fit._points_inputs(dict(coords=pts, mv=mv, anchor=np.zeros(40, dtype=np.int64), joints=mv), pb["p"], 2, ())


def test_host_layout_mirrors_the_library_contract():
    """Groups by first appearance, members in the caller's order, g x g column-major blocks one after the other."""
    from spamtree_amd import fit
    groups, off = fit._joint_layout(np.array([5, 3, 5, 9, 3, 5]))
    assert [g.tolist() for g in groups] == [[0, 2, 5], [1, 4], [3]] and off.tolist() == [0, 9, 13, 14]
    blocks = fit._unpack_joint(np.arange(14.0), groups, off)
    assert blocks[0][1, 0] == 1.0 and blocks[0][0, 1] == 3.0 and blocks[1].shape == (2, 2) and blocks[2][0, 0] == 13.0
    same = fit._unpack_joint(np.arange(8.0), *fit._joint_layout(np.array([1, 1, 2, 2])))
    assert same.shape == (2, 2, 2)
