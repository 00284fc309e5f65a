"""GPU parity of ``GroundElevation`` (``transforms.GroundElevation`` -> ``ground.ground_mask`` /
``fit_ground_plane`` / ``ground_elevation`` on ``csrc/ground.hip``).

Bars.  Masks, trimmed indices, inlier counts per hypothesis, the best hypothesis and every tie rule
are EXACT: against the reference's own output (tests/golden/ground.npz, made by
tests/golden/make_golden_ground.py from the reference's source) and against the f64 restatement
tests/ground_reference.py on generated clouds.  Exact counts are asked only where no
(hypothesis, point) residual lies within 1e-5 of the threshold: the fixture's triplets were drawn
under that condition (checked for every pair by the golden script and by
tests/test_ground_reference_cpu.py); generated clouds check it themselves before they compare.

The plane and the elevation have a measured bound: the reference's f32 result deviates from the
f64 closed form by 9.43e-08 (plane) and 1.58e-07 (elevation), max |diff| / max |f64 value| over the
worst fixture case (measured on the CPU by tests/test_ground_reference_cpu.py); the kernels get
4x that against the golden, 3.77e-07 and 6.32e-07.  The reference's figures are recorded in
profiles/r10a_ground_errors.txt; the kernels' own are printed by every test before it asserts
(pytest -s) and belong in the same file - they have not been recorded on an MI355X yet.

Shapes: N = 1, 63, 65, 257 and 100 003 for the filters (below / above a wave, several workgroups,
odd), 100 000 points in one cell, 300 000 shuffled points over 1 cell and over about 10^5 cells,
z_threshold alone with M of the order of N = 300 000."""
import numpy as np
import pytest
import torch

import ground_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

_Z = None
_REF = {}


def fixture_case(case):
    global _Z
    if _Z is None:
        _Z = load_golden("ground.npz")
    return R.load_fixture_case(_Z, case)


def fixture_reference(case):
    if case not in _REF:
        f = fixture_case(case)
        _REF[case] = R.ground_elevation_reference(f["pos"], f["samples"], scale=f["scale"], **f["params"])
    return _REF[case]


def G():
    from superpoint_transformer_amd import ground
    return ground


def on(dev, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def trimmed_indices(dev, pos, **kw):
    vert = kw.pop("verticality", None)
    t = G().ground_mask(on(dev, pos), verticality=on(dev, vert), **kw)
    idx = t.indices()
    assert idx.dtype == torch.long and idx.is_cuda and t.count.is_cuda
    return idx.cpu().numpy(), t


# ---- the fixture -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES)
def test_fixture_masks_and_indices_match_the_reference(case, dev):
    f = fixture_case(case)
    prm = f["params"]
    if "z_threshold" in prm:
        t = G().ground_mask(on(dev, f["pos"]), z_threshold=prm["z_threshold"])
        assert np.array_equal(t.mask().cpu().numpy(), f["mask_z"])
    if "xy_grid" in prm:
        t = G().ground_mask(on(dev, f["pos"]), xy_grid=prm["xy_grid"])
        assert np.array_equal(t.mask().cpu().numpy(), f["mask_cell"])
    idx, _ = trimmed_indices(dev, f["pos"], **prm)
    assert np.array_equal(idx, f["index"])


@pytest.mark.parametrize("case", R.CASES)
def test_fixture_inlier_counts_for_fixed_samples(case, dev):
    f, r = fixture_case(case), fixture_reference(case)
    assert r["closest"] > R.MARGIN
    pos = on(dev, f["pos"])
    t = G().ground_mask(pos, **f["params"])
    plane = G().fit_ground_plane(pos, t, samples=on(dev, f["samples"]))
    assert np.array_equal(plane.counts.cpu().numpy().astype(np.int64), r["counts"])
    assert plane.best_index == r["best"] and plane.best_count == int(r["counts"].max())
    assert plane.num_trimmed == f["index"].size and plane.num_valid == int(r["valid"].sum())
    assert plane.num_refit == int(r["inliers"].sum()) == int(f["inliers"].sum())
    dk = R.relative_deviation(plane.plane, r["plane"])
    print(f"\nground fixture '{case}' (fixed samples): kernel plane vs f64 closed form {dk:.3e}")
    assert dk <= R.BOUND_PLANE


@pytest.mark.parametrize("case", R.CASES)
def test_fixture_plane_and_elevation_within_the_measured_bound(case, dev):
    """The transform as a user calls it (seeded hypotheses) against the golden; bound and recorded
    figures: profiles/r10a_ground_errors.txt."""
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import GroundElevation
    f, r = fixture_case(case), fixture_reference(case)
    t = GroundElevation(scale=f["scale"], **f["params"])
    data = t(Data(pos=on(dev, f["pos"])))
    assert data.elevation.shape == (f["pos"].shape[0], 1) and data.elevation.dtype == torch.float32
    rec = t.ground_plane_
    assert rec.num_trimmed == f["index"].size
    assert rec.best_count == int(f["inliers"].sum()), "the seeded hypotheses missed the ground"
    got = data.elevation.cpu().numpy()
    dp, de = R.relative_deviation(rec.plane, f["plane"]), R.relative_deviation(got, f["elevation"])
    kp, ke = R.relative_deviation(rec.plane, r["plane"]), R.relative_deviation(got, r["elevation"])
    print(f"\nground fixture '{case}': kernel vs golden: plane {dp:.3e}, elevation {de:.3e}; "
          f"kernel vs f64 closed form: plane {kp:.3e}, elevation {ke:.3e}")
    assert dp <= R.BOUND_PLANE and de <= R.BOUND_ELEVATION
    assert kp <= R.BOUND_PLANE and ke <= R.BOUND_ELEVATION


# ---- filters on generated clouds -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257, 100_003])
def test_filters_match_the_restatement(n, dev):
    rng = np.random.default_rng(500 + n)
    pos, _ = R.tilted_cloud(rng, n - n // 3, n // 3, extent=30.0, origin=(1.5, -2.0))
    vert = rng.random(n).astype(np.float32)
    combos = [dict(), dict(z_threshold=0.75), dict(xy_grid=1.0), dict(xy_grid=0.3, z_threshold=0.75),
              dict(verticality_threshold=0.25, verticality=vert),
              dict(xy_grid=2.5, z_threshold=1.5, verticality_threshold=0.5, verticality=vert)]
    for kw in combos:
        idx, t = trimmed_indices(dev, pos, **dict(kw))
        ref = np.nonzero(R.ground_mask(pos, **kw))[0]
        assert np.array_equal(idx, ref), (n, sorted(kw))
        assert int(t.count) == ref.size


def torch_cells(pos, grid):
    return (pos[:, 0].div(grid, rounding_mode="trunc").long(), pos[:, 1].div(grid, rounding_mode="trunc").long())


def torch_cell_winners(pos, grid):
    """Winners by torch's own ``div(..., rounding_mode='trunc')`` (partition.py:35-36); z holds
    distinct values, so the winner of a cell is unambiguous.  ``grid`` is a Python number or a
    0-dim tensor on ``pos``'s device."""
    i, j = torch_cells(pos, grid)
    i, j = i - i.min(), j - j.min()
    cell = i * (j.max() + 1) + j
    order = torch.argsort(pos[:, 2], stable=True)
    order = order[torch.argsort(cell[order], stable=True)]
    first = torch.ones_like(order, dtype=torch.bool)
    first[1:] = cell[order][1:] != cell[order][:-1]
    return torch.sort(order[first]).values


@pytest.mark.parametrize("grid", [1.0, 0.3, 2.5])
def test_cell_boundaries_and_the_origin(grid, dev):
    """Points exactly on cell boundaries, one ulp to either side of them, and around the origin:
    membership must be torch's trunc of the IEEE f32 quotient (a floor, or a product with
    1 / grid, moves some of them).

    Which torch.  ``div(number, rounding_mode='trunc')`` is that quotient on the CPU, where the
    golden fixture was made.  On the device torch's kernel takes a shortcut for a Python-number
    divisor: it multiplies by ``1 / grid`` rounded to f32 ("may lose one bit of precision" in its
    source), which puts boundary points of grid = 0.3 into the neighbouring cell.  That is the
    product the kernels must NOT compute.  So the kernels are held to torch's CPU result; how many
    points torch's device kernel moves, with a number divisor and with the divisor as a 0-dim device
    tensor (no shortcut in its source), is printed."""
    k = np.arange(-40, 41, dtype=np.float32)
    edge = k * np.float32(grid)
    vals = np.concatenate((edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf)),
                           np.float32([0.0, -0.0, 1e-30, -1e-30, 0.999999 * grid, -0.999999 * grid])))
    rng = np.random.default_rng(7)
    x, y = np.meshgrid(vals, vals)
    n = x.size
    z = rng.permutation(n).astype(np.float32)                  # distinct heights
    pos = np.stack((x.ravel(), y.ravel(), z), axis=1).astype(np.float32)
    pos = pos[rng.permutation(n)]
    cpos, dpos = torch.from_numpy(pos), on(dev, pos)
    idx, _ = trimmed_indices(dev, pos, xy_grid=grid)
    ci, cj = torch_cells(cpos, grid)
    si, sj = (t.cpu() for t in torch_cells(dpos, grid))
    ti, tj = (t.cpu() for t in torch_cells(dpos, torch.tensor(grid, dtype=torch.float32, device=dev)))
    print(f"\ngrid {grid}: of {n} points, torch's device kernel with a number divisor puts "
          f"{int(((si != ci) | (sj != cj)).sum())} into another cell than torch on the CPU; with a "
          f"tensor divisor {int(((ti != ci) | (tj != cj)).sum())}")
    assert np.array_equal(idx, torch_cell_winners(cpos, grid).numpy())
    assert np.array_equal(idx, np.nonzero(R.filter_local_z_min(pos, grid))[0])
    # the two cells around the origin are one: fewer cells than a floor would make
    i, _ = R.cell_coords(pos, grid)
    assert np.unique(i).size < np.unique(np.floor(pos[:, 0].astype(np.float64) / grid)).size


def test_one_cell_repeated_minima_lowest_index_wins(dev):
    n = 100_000
    rng = np.random.default_rng(11)
    pos = np.empty((n, 3), dtype=np.float32)
    pos[:, :2] = rng.uniform(0.05, 0.95, (n, 2))
    pos[:, 2] = rng.integers(0, 4, n).astype(np.float32)       # about 25 000 points share the minimum
    pos[:777, 2] += 1.0                                        # the first of them is not point 0
    pos[5000, 2] = -0.0
    first = int(np.nonzero(pos[:, 2] == 0)[0][0])
    assert first >= 777 and (pos[:, 2] == 0).sum() > 10_000
    idx, _ = trimmed_indices(dev, pos, xy_grid=1.0)
    assert idx.tolist() == [first]
    assert np.array_equal(idx, np.nonzero(R.filter_local_z_min(pos, 1.0))[0])


@pytest.mark.parametrize("extent,cells", [(0.9, 1), (316.0, 100_000)])
def test_table_sizes_300k_shuffled(extent, cells, dev):
    n = 300_000
    rng = np.random.default_rng(13)
    pos = np.empty((n, 3), dtype=np.float32)
    lo = 0.05 if cells == 1 else -extent / 2
    pos[:, :2] = rng.uniform(lo, lo + extent, (n, 2))
    pos[:, 2] = rng.normal(0, 1, n)
    idx, _ = trimmed_indices(dev, pos, xy_grid=1.0)
    ref = np.nonzero(R.filter_local_z_min(pos, 1.0))[0]
    assert np.array_equal(idx, ref)
    assert (idx.size == 1) if cells == 1 else (0.85 * cells < idx.size <= 1.02 * cells)


def test_verticality_threshold_is_applied(dev):
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import GroundElevation
    rng = np.random.default_rng(17)
    pos, is_ground = R.tilted_cloud(rng, 4000, 2000)
    vert = np.where(is_ground, rng.uniform(0.0, 0.2, 6000), rng.uniform(0.3, 1.0, 6000)).astype(np.float32)
    idx, _ = trimmed_indices(dev, pos, verticality=vert, verticality_threshold=0.25)
    assert np.array_equal(idx, np.nonzero(is_ground)[0])
    t = GroundElevation(verticality_threshold=0.25, scale=1.0)
    data = t(Data(pos=on(dev, pos), verticality=on(dev, vert.reshape(-1, 1))))
    assert t.ground_plane_.num_trimmed == t.ground_plane_.best_count == 4000
    assert float(data.elevation.cpu().abs().numpy()[is_ground].max()) < 1e-6
    # without the filter the clutter is part of the trimmed set
    assert GroundElevation(scale=1.0)(Data(pos=on(dev, pos))) is not None
    assert G().ground_mask(on(dev, pos)).indices().numel() == 6000


def test_z_threshold_alone_keeps_most_points(dev):
    n = 300_000
    rng = np.random.default_rng(19)
    pos, is_ground = R.tilted_cloud(rng, 250_000, 50_000, extent=60.0)
    idx, t = trimmed_indices(dev, pos, z_threshold=3.5)
    ref = np.nonzero(R.filter_z(pos, 3.5))[0]
    assert np.array_equal(idx, ref) and idx.size > 0.8 * n
    # and the fit on that many points: every ground point is an inlier, the refit is the f64 one
    plane = G().fit_ground_plane(on(dev, pos), t, seed=3)
    ground_in = is_ground[ref]
    assert plane.best_count == int(ground_in.sum()) == plane.num_refit
    assert R.relative_deviation(plane.plane, R.refit(pos[ref][ground_in])) < 1e-9


# ---- hypotheses ----------------------------------------------------------------------------------
def test_degenerate_triplets_and_the_tie_rule(dev):
    rng = np.random.default_rng(23)
    pos, _ = R.tilted_cloud(rng, 150, 50)
    n = pos.shape[0]
    pos[0, :2], pos[1, :2], pos[2, :2] = (0.0, 0.0), (1.0, 2.0), (2.0, 4.0)      # collinear in XY
    good = np.nonzero(np.arange(n) > 2)[0]
    a, b = rng.choice(good, 3, replace=False), rng.choice(good, 3, replace=False)
    samples = np.array([[5, 6, 6], [0, 1, 2], [3, 4, n], [-1, 3, 4], a, b, a, [7, 7, 7], a[::-1]], dtype=np.int64)
    dpos = on(dev, pos)
    t = G().ground_mask(dpos)
    r = R.ground_elevation_reference(pos, samples, scale=1.0)
    assert r["valid"].tolist() == [False, False, False, False, True, True, True, False, True]
    plane = G().fit_ground_plane(dpos, t, samples=on(dev, samples))
    counts = plane.counts.cpu().numpy()
    assert counts[[0, 1, 2, 3, 7]].tolist() == [-1] * 5
    assert counts[4] == counts[6] >= 3 and plane.num_valid == 4
    if r["closest"] > R.MARGIN:
        assert np.array_equal(counts.astype(np.int64), r["counts"])
    # hypotheses 4 and 6 are the same triplet: whichever of {4, 5} scores best, 6 never wins
    assert plane.best_index == int(np.argmax(counts)) and plane.best_index in (4, 5)
    only_ties = G().fit_ground_plane(dpos, t, samples=on(dev, np.stack([samples[1], a, a, a])))
    assert only_ties.best_index == 1 and only_ties.counts.cpu().tolist()[0] == -1
    with pytest.raises(ValueError, match="no valid hypothesis"):
        G().fit_ground_plane(dpos, t, samples=on(dev, samples[[0, 1, 2, 3, 7]]))


def test_generated_cloud_counts_match_the_restatement(dev):
    """Several workgroups of trimmed points (M = 40 000) and a partial last wave."""
    rng = np.random.default_rng(29)
    pos, is_ground = R.tilted_cloud(rng, 30_011, 10_000, extent=40.0, origin=(-3.0, 8.0))
    m = pos.shape[0]
    g = np.nonzero(is_ground)[0]
    samples = np.stack([rng.choice(g, 3, replace=False) for _ in range(40)]
                       + [rng.choice(m, 3, replace=False) for _ in range(24)])
    planes, valid = R.hypothesis_planes(pos, samples)
    counts, _ = R.score(pos, planes, valid)
    keep = np.array([R.score(pos, planes[h:h + 1], valid[h:h + 1])[1] > R.MARGIN for h in range(len(samples))])
    assert keep.sum() >= 40                                     # the exactness condition, per hypothesis
    dpos = on(dev, pos)
    plane = G().fit_ground_plane(dpos, G().ground_mask(dpos), samples=on(dev, samples[keep]))
    assert np.array_equal(plane.counts.cpu().numpy().astype(np.int64), counts[keep])
    assert plane.best_index == R.best_hypothesis(counts[keep])
    assert R.relative_deviation(plane.plane, R.refit(pos[is_ground])) < 1e-9


# ---- reproducibility, errors, bypass -----------------------------------------------------------------
def test_two_runs_with_the_same_seed_are_bitwise_equal(dev):
    rng = np.random.default_rng(31)
    pos, _ = R.tilted_cloud(rng, 200_000, 100_000, extent=120.0)
    dpos = on(dev, pos)
    runs = [G().ground_elevation(dpos, z_threshold=5.0, xy_grid=1.0, scale=4.0, random_state=7)
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1].status.view(torch.int64), runs[1][1].status.view(torch.int64))
    assert torch.equal(runs[0][1].counts, runs[1][1].counts)
    # the seed is used: without the cell filter the trimmed set holds clutter, and which triplets
    # touch it depends on the draw
    t = G().ground_mask(dpos, z_threshold=5.0)
    a, b, c = (G().fit_ground_plane(dpos, t, seed=s).counts for s in (7, 7, 8))
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_errors(dev):
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import GroundElevation
    rng = np.random.default_rng(37)
    pos, _ = R.tilted_cloud(rng, 500, 100)
    dpos = on(dev, pos)
    with pytest.raises(ValueError, match="a plane needs 3"):     # M < 3: only the lowest point is left
        GroundElevation(z_threshold=1e-12)(Data(pos=dpos))
    far = pos.copy()
    far[0, 0] = 3.0e7                                            # one far outlier
    with pytest.raises(ValueError, match=r"xy_grid = 0\.01 .* cells \(x cells"):
        GroundElevation(xy_grid=0.01)(Data(pos=on(dev, far)))
    with pytest.raises(ValueError, match="does not have a 'verticality' attribute"):
        GroundElevation(verticality_threshold=0.5)(Data(pos=dpos))
    with pytest.raises(NotImplementedError, match="knn"):
        GroundElevation(model="knn")(Data(pos=dpos))
    with pytest.raises(NotImplementedError, match="mlp"):
        GroundElevation(model="mlp")(Data(pos=dpos))
    with pytest.raises(RuntimeError, match="MI355X only"):
        GroundElevation(xy_grid=1.0)(Data(pos=torch.from_numpy(pos)))


def test_scale_not_positive_is_the_identity(dev):
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import GroundElevation
    data = Data(pos=torch.zeros(4, 3, device=dev))
    for scale in (0, -1.0):
        out = GroundElevation(xy_grid=1.0, model="mlp", scale=scale)(data)
        assert out is data and "elevation" not in data and data.keys == ["pos"]
