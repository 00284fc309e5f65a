"""CPU suite: the f64 restatement of ``GroundElevation`` (tests/ground_reference.py) pinned on the
reference's own output (tests/golden/ground.npz, written by tests/golden/make_golden_ground.py).

Masks, trimmed indices and the inlier set are EXACT.  The plane and the elevation differ, because
the reference fits in f32 (scikit-learn keeps its input's dtype) and the restatement in f64: the
deviations measured here are the yardsticks of the GPU suite (ground_reference.YARDSTICK_*,
recorded in profiles/r10a_ground_errors.txt); this file pins them from above and prints them
(pytest -s)."""
import numpy as np
import pytest

import ground_reference as R
from conftest import load_golden

_Z = None


def fixture_case(case):
    global _Z
    if _Z is None:
        _Z = load_golden("ground.npz")
    return R.load_fixture_case(_Z, case)


@pytest.mark.parametrize("case", R.CASES)
def test_filters_match_the_reference(case):
    f = fixture_case(case)
    prm = f["params"]
    mask = np.ones(f["pos"].shape[0], dtype=bool)
    if "z_threshold" in prm:
        mz = R.filter_z(f["pos"], prm["z_threshold"])
        assert np.array_equal(mz, f["mask_z"])
        mask &= mz
    if "xy_grid" in prm:
        mc = R.filter_local_z_min(f["pos"], prm["xy_grid"])
        assert np.array_equal(mc, f["mask_cell"])
        mask &= mc
    assert np.array_equal(R.ground_mask(f["pos"], **prm), mask)
    assert np.array_equal(np.nonzero(mask)[0], f["index"])
    assert f["index"].size >= 100


def test_the_fixture_is_what_the_issue_asks_for():
    f = fixture_case("grid")
    pos, ground = f["pos"], f["is_ground"]
    assert 5000 <= pos.shape[0] <= 7000
    assert pos[:, 0].min() < -1 < 1 < pos[:, 0].max() and pos[:, 1].min() < -1 < 1 < pos[:, 1].max()
    # the ground lies exactly on one plane: the f64 closed form leaves only the f32 rounding of z
    plane = R.refit(pos[ground].astype(np.float64))
    assert R.residuals(pos[ground], plane).max() < 2e-7
    # clutter at least 5 cm above, a pit below
    rest = pos[~ground].astype(np.float64)
    dz = rest[:, 2] - (plane[0] * rest[:, 0] + plane[1] * rest[:, 1] + plane[2])
    assert dz[dz > 0].min() >= 0.05 - 1e-6 and (dz < -0.25).sum() >= 20
    # cells that hold clutter only
    assert (~ground[f["index"]]).sum() >= 5
    # cells around the origin exist on all four sides
    i, j = R.cell_coords(pos, 1.0)
    assert {(-1, -1), (-1, 1), (1, -1), (1, 1)} <= set(zip(np.sign(i).tolist(), np.sign(j).tolist()))


@pytest.mark.parametrize("case", R.CASES)
def test_no_residual_near_the_threshold(case):
    """The condition that lets the GPU suite ask for exact inlier counts: for the fixture's
    triplets, EVERY (hypothesis, trimmed point) residual is at least MARGIN from the threshold."""
    f = fixture_case(case)
    trimmed = f["pos"][f["index"]]
    planes, valid = R.hypothesis_planes(trimmed, f["samples"])
    counts, closest = R.score(trimmed, planes, valid)
    assert valid.all()
    assert closest > R.MARGIN
    assert counts.max() == f["is_ground"][f["index"]].sum()


@pytest.mark.parametrize("case", R.CASES)
def test_plane_and_elevation_against_the_reference(case):
    f = fixture_case(case)
    r = R.ground_elevation_reference(f["pos"], f["samples"], scale=f["scale"], **f["params"])
    assert np.array_equal(r["index"], f["index"])
    assert np.array_equal(r["inliers"], f["inliers"].astype(bool)), "not the reference's inlier set"
    dp = R.relative_deviation(f["plane"], r["plane"])
    de = R.relative_deviation(f["elevation"], r["elevation"])
    print(f"\nground fixture '{case}': reference (f32 sklearn) vs f64 closed form: "
          f"plane {dp:.3e}, elevation {de:.3e}")
    assert dp <= R.YARDSTICK_PLANE and de <= R.YARDSTICK_ELEVATION


def test_yardsticks_are_the_measured_worst_case():
    """YARDSTICK_* are the worst case's figures rounded up in the third digit, not loose ceilings."""
    dp = de = 0.0
    for case in R.CASES:
        f = fixture_case(case)
        r = R.ground_elevation_reference(f["pos"], f["samples"], scale=f["scale"], **f["params"])
        dp = max(dp, R.relative_deviation(f["plane"], r["plane"]))
        de = max(de, R.relative_deviation(f["elevation"], r["elevation"]))
    assert R.YARDSTICK_PLANE / 1.01 < dp <= R.YARDSTICK_PLANE
    assert R.YARDSTICK_ELEVATION / 1.01 < de <= R.YARDSTICK_ELEVATION


def test_restatement_rules():
    # trunc, not floor: the two cells around the origin are one
    pos = np.array([[-0.5, 0.5, 1.0], [0.5, -0.5, 0.5], [-1.0, 0.0, 0.0], [1.0, 0.0, 2.0]], dtype=np.float32)
    assert np.array_equal(R.filter_local_z_min(pos, 1.0), [False, True, True, True])
    # equal minima: the lowest index; -0.0 and +0.0 are equal
    pos = np.array([[0.1, 0.1, 0.0], [0.2, 0.2, -0.0], [0.3, 0.3, 0.0]], dtype=np.float32)
    assert np.array_equal(R.filter_local_z_min(pos, 1.0), [True, False, False])
    # repeated index, collinear triplet, out of range
    t = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 1]], dtype=np.float64)
    planes, valid = R.hypothesis_planes(t, [[0, 1, 1], [0, 1, 2], [0, 1, 3], [0, 1, 4]])
    assert valid.tolist() == [False, False, True, False]
    assert np.allclose(planes[2], [0, 1, 0])
    counts, _ = R.score(t, planes, valid)
    assert counts.tolist() == [-1, -1, 4, -1] and R.best_hypothesis(counts) == 2
    assert R.best_hypothesis(np.array([-1, 3, 3])) == 1 and R.best_hypothesis(np.array([-1, -1])) == -1
    assert R.samples_from_u(np.array([[0.0, 0.5, 0.99999994]], dtype=np.float32), 10).tolist() == [[0, 5, 9]]
