"""f64 numpy restatement of ``GroundElevation`` with ``model='ransac'``
(src/transforms/point.py:268-326, src/utils/ground.py:25-131, src/utils/partition.py:17-50): the
three filters, the scoring of GIVEN hypotheses, the least-squares refit on the best one's inliers
and the elevation.  Pinned on the reference's own output (tests/golden/ground.npz, written by
tests/golden/make_golden_ground.py) by tests/test_ground_reference_cpu.py; the GPU suite
(tests/test_ground_gpu.py) compares the kernels of csrc/ground.hip against it.

What is f32 in the reference stays f32 here, because it decides set membership: the cell
coordinate ``trunc(x / grid)`` (an IEEE f32 division), ``z - z.min() < z_threshold`` and
``verticality < threshold``.  Everything after the trimmed set is f64.

Rules the reference leaves open: the lowest point of a cell is, among equal z, the one with the
lowest index; the best hypothesis is, among equal counts, the one with the lowest index; a
triplet is degenerate when it repeats a point or when the sine of the angle between two edges
of its XY triangle is at most 1e-9.

Bounds of the plane and of the elevation.  The reference fits in f32 (scikit-learn keeps the
dtype of its input); its deviation from the f64 closed form on the fixture, as
``max |diff| / max |f64 value|`` over the worst case, is YARDSTICK_PLANE / YARDSTICK_ELEVATION
below (measured by tests/test_ground_reference_cpu.py, recorded in
profiles/r10a_ground_errors.txt).  The kernels get 4x that, the margin of
tests/test_adjacency_gpu.py."""
import numpy as np

RESIDUAL_THRESHOLD = 1e-3
MARGIN = 1e-5                      # no fixture residual lies this close to the threshold

# the reference's own deviation from the f64 closed form (profiles/r10a_ground_errors.txt)
YARDSTICK_PLANE = 9.43e-08
YARDSTICK_ELEVATION = 1.58e-07
BOUND_PLANE = 4 * YARDSTICK_PLANE
BOUND_ELEVATION = 4 * YARDSTICK_ELEVATION

CASES = ("both", "grid", "z")


def relative_deviation(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- filters -------------------------------------------------------------------------------
def cell_coords(pos, grid):
    """(i, j) int64 of every point: trunc of the f32 quotient (partition.py:35-36)."""
    p = np.asarray(pos, dtype=np.float32)
    g = np.float32(grid)
    return np.trunc(p[:, 0] / g).astype(np.int64), np.trunc(p[:, 1] / g).astype(np.int64)


def filter_z(pos, threshold):
    z = np.asarray(pos, dtype=np.float32)[:, 2]
    return (z - z.min()) < np.float32(threshold)


def filter_verticality(verticality, threshold):
    return np.asarray(verticality, dtype=np.float32).reshape(-1) < np.float32(threshold)


def filter_local_z_min(pos, grid):
    """Lowest point of every XY cell, over ALL points; equal z: lowest index."""
    p = np.asarray(pos, dtype=np.float32)
    i, j = cell_coords(p, grid)
    i, j = i - i.min(), j - j.min()
    cell = i * (j.max() + 1) + j
    z = p[:, 2] + np.float32(0)                                  # -0.0 -> +0.0
    order = np.lexsort((np.arange(p.shape[0]), z, cell))         # by cell, then z, then index
    first = np.ones(order.size, dtype=bool)
    first[1:] = cell[order][1:] != cell[order][:-1]
    mask = np.zeros(p.shape[0], dtype=bool)
    mask[order[first]] = True
    return mask


def ground_mask(pos, z_threshold=None, verticality=None, verticality_threshold=None, xy_grid=None):
    mask = np.ones(np.asarray(pos).shape[0], dtype=bool)
    if z_threshold is not None:
        mask &= filter_z(pos, z_threshold)
    if verticality_threshold is not None:
        mask &= filter_verticality(verticality, verticality_threshold)
    if xy_grid:
        mask &= filter_local_z_min(pos, xy_grid)
    return mask


# ---- hypotheses ----------------------------------------------------------------------------
def samples_from_u(u, m):
    """min(floor(u M), M - 1) for u [H, 3] f32 in [0, 1)."""
    s = np.floor(np.asarray(u, dtype=np.float32).astype(np.float64) * float(m)).astype(np.int64)
    return np.minimum(s, m - 1)


def hypothesis_planes(trimmed, samples):
    """planes [H, 3] f64 (NaN rows for invalid triplets) and valid [H] of the triplets
    ``samples`` [H, 3] into ``trimmed`` [M, 3]."""
    t = np.asarray(trimmed, dtype=np.float64)
    s = np.asarray(samples, dtype=np.int64).reshape(-1, 3)
    m = t.shape[0]
    valid = ((s >= 0) & (s < m)).all(axis=1)
    valid &= (s[:, 0] != s[:, 1]) & (s[:, 0] != s[:, 2]) & (s[:, 1] != s[:, 2])
    planes = np.full((s.shape[0], 3), np.nan)
    for h in np.nonzero(valid)[0]:
        p0, p1, p2 = t[s[h, 0]], t[s[h, 1]], t[s[h, 2]]
        d1, d2 = p1 - p0, p2 - p0
        det = d1[0] * d2[1] - d2[0] * d1[1]
        n1, n2 = d1[0] * d1[0] + d1[1] * d1[1], d2[0] * d2[0] + d2[1] * d2[1]
        if not det * det > 1e-18 * (n1 * n2):
            valid[h] = False
            continue
        a = (d1[2] * d2[1] - d2[2] * d1[1]) / det
        b = (d1[0] * d2[2] - d2[0] * d1[2]) / det
        c = p0[2] - (a * p0[0] + b * p0[1])
        if not np.isfinite([a, b, c]).all():
            valid[h] = False
            continue
        planes[h] = (a, b, c)
    return planes, valid


def residuals(trimmed, plane):
    t = np.asarray(trimmed, dtype=np.float64)
    return np.abs(t[:, 2] - ((plane[0] * t[:, 0] + plane[1] * t[:, 1]) + plane[2]))


def score(trimmed, planes, valid, threshold=RESIDUAL_THRESHOLD):
    """counts [H] int64 (-1 for invalid hypotheses) and the smallest | residual - threshold |
    over every (valid hypothesis, point) pair."""
    counts = np.full(planes.shape[0], -1, dtype=np.int64)
    closest = np.inf
    for h in np.nonzero(valid)[0]:
        r = residuals(trimmed, planes[h])
        counts[h] = int((r < threshold).sum())
        if r.size:
            closest = min(closest, float(np.abs(r - threshold).min()))
    return counts, closest


def best_hypothesis(counts):
    """Largest count, lowest index among equals; -1 when none is valid."""
    return int(np.argmax(counts)) if counts.size and counts.max() >= 0 else -1


def refit(inliers):
    """Least-squares plane of the inlier points (sklearn's final LinearRegression), f64:
    centred normal equations in closed form."""
    t = np.asarray(inliers, dtype=np.float64)
    mean = t.mean(axis=0)
    d = t - mean
    cxx, cxy, cyy = (d[:, 0] * d[:, 0]).sum(), (d[:, 0] * d[:, 1]).sum(), (d[:, 1] * d[:, 1]).sum()
    cxz, cyz = (d[:, 0] * d[:, 2]).sum(), (d[:, 1] * d[:, 2]).sum()
    det = cxx * cyy - cxy * cxy
    a = (cxz * cyy - cyz * cxy) / det
    b = (cyz * cxx - cxz * cxy) / det
    return np.array([a, b, mean[2] - (a * mean[0] + b * mean[1])])


def elevation(pos, plane, scale):
    p = np.asarray(pos, dtype=np.float64)
    return ((p[:, 2] - ((plane[0] * p[:, 0] + plane[1] * p[:, 1]) + plane[2])) / scale).reshape(-1, 1)


def ground_elevation_reference(pos, samples, z_threshold=None, verticality=None,
                               verticality_threshold=None, xy_grid=None, scale=3.0,
                               threshold=RESIDUAL_THRESHOLD):
    """The whole transform for given triplets.  Returns a dict: mask, index, planes, valid,
    counts, closest, best, inliers (mask over the trimmed set), plane, elevation."""
    p = np.asarray(pos, dtype=np.float32)
    mask = ground_mask(p, z_threshold, verticality, verticality_threshold, xy_grid)
    index = np.nonzero(mask)[0]
    trimmed = p[index].astype(np.float64)
    planes, valid = hypothesis_planes(trimmed, samples)
    counts, closest = score(trimmed, planes, valid, threshold)
    best = best_hypothesis(counts)
    out = dict(mask=mask, index=index, planes=planes, valid=valid, counts=counts, closest=closest,
               best=best, inliers=None, plane=None, elevation=None)
    if best >= 0:
        out["inliers"] = residuals(trimmed, planes[best]) < threshold
        out["plane"] = refit(trimmed[out["inliers"]])
        out["elevation"] = elevation(p, out["plane"], scale)
    return out


# ---- the fixture -----------------------------------------------------------------------------
CASE_PARAMS = {"both": dict(z_threshold=1.5, xy_grid=2.0), "grid": dict(xy_grid=1.0),
               "z": dict(z_threshold=1.5)}
SCALE = 3.0


def load_fixture_case(z, case):
    """One parameter set of tests/golden/ground.npz as numpy arrays."""
    out = dict(pos=np.asarray(z["pos"], dtype=np.float32), is_ground=np.asarray(z["is_ground"]).astype(bool),
               params=CASE_PARAMS[case], scale=SCALE)
    for k in ("mask_z", "mask_cell", "index", "plane", "elevation", "samples", "inliers"):
        key = f"{case}_{k}"
        if key in z:
            out[k] = np.asarray(z[key])
    out["index"] = out["index"].astype(np.int64)
    out["samples"] = out["samples"].astype(np.int64)
    return out


# ---- generated clouds of the GPU suite -------------------------------------------------------
def tilted_cloud(rng, n_ground, n_clutter, extent=20.0, origin=(0.0, 0.0), plane=(0.03, -0.02, 0.5)):
    """Ground exactly on a plane (evaluated in f64, rounded to f32) and clutter at least 5 cm
    above it, around ``origin``; shuffled.  Returns (pos f32, is_ground)."""
    n = n_ground + n_clutter
    xy = (rng.random((n, 2)) - 0.5) * extent + np.asarray(origin)
    xy = xy.astype(np.float32)
    z = plane[0] * xy[:, 0].astype(np.float64) + plane[1] * xy[:, 1].astype(np.float64) + plane[2]
    z[n_ground:] += 0.05 + rng.random(n_clutter) * 2.5
    pos = np.concatenate((xy, z.astype(np.float32)[:, None]), axis=1)
    is_ground = np.arange(n) < n_ground
    perm = rng.permutation(n)
    return pos[perm], is_ground[perm]
