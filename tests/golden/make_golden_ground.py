"""Golden fixture for ``GroundElevation``, produced by the REFERENCE'S OWN
``GroundElevation.__init__`` / ``_process`` (src/transforms/point.py:185-326, the class cut out
of the file with ``ast`` - unmodified - because the module pulls the whole model zoo at import)
and the verbatim-imported src/utils/ground.py (``filter_by_z_distance_of_global_min``,
``filter_by_local_z_min``, ``filter_by_verticality``, ``single_plane_model``) and
src/utils/partition.py (``xy_partition``).

The CPU branch of ``single_plane_model`` runs: scikit-learn's ``RANSACRegressor`` (1.7.2 here);
``torch_ransac3d`` is not installed and only the GPU branch needs it.  Stand-ins: the imports
ground.py / partition.py do not use on that branch (hydra, omegaconf, tqdm, torch_ransac3d,
src.utils.hydra) are empty modules; ``torch_scatter.scatter_min`` and torch_geometric's
``consecutive_cluster`` are the restatements of oracle/spt_oracle.py ("[third-party restated]").

The cloud (about 6 k points, x in [-12, 14], y in [-9, 11]: both straddle the origin):
  * ground exactly on a tilted plane, evaluated in f64 at the f32 (x, y) and rounded to f32;
  * clutter 5 cm .. 3 m above it, and one corner that holds clutter ONLY (no ground point there:
    the cell filter keeps clutter points);
  * a small pit 0.3 .. 0.6 m below the plane (it sets the global z minimum);
  * no two points of a cell share the cell's lowest z (asserted).

Three parameter sets: both filters (z_threshold 1.5, xy_grid 2), xy_grid 1 only, z_threshold 1.5
only; scale 3.  Stored per set: each filter's mask, the trimmed indices, sklearn's fitted
(a, b, c), its inlier mask over the trimmed set and the elevation.  The script asserts that
sklearn's inlier set is exactly the planar ground of the trimmed set.

Also stored per set: ``samples`` [H, 3], triplets into the trimmed set for the tests that fix the
hypotheses (mixed: all-ground triplets and triplets with clutter / pit points).  They are drawn
by rejection so that NO (hypothesis, trimmed point) residual lies within 1e-5 of the residual
threshold 1e-3 - checked below for every pair with tests/ground_reference.py - which is what lets
the GPU suite ask for exact inlier counts.

Usage (build container only): python tests/golden/make_golden_ground.py
"""
import ast
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import ground_reference as R  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

REF = mg.REF
NUM_SAMPLES = 48


def load_reference():
    U, _ = mg.install_reference_import_hooks()
    sys.modules["torch_geometric.nn.pool.consecutive"].consecutive_cluster = O.consecutive_cluster
    for name in ("hydra", "omegaconf", "tqdm", "torch_ransac3d", "torch_ransac3d.plane",
                 "src.utils.hydra"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["src.utils.hydra"].init_config = None
    sys.modules["omegaconf"].OmegaConf = getattr(sys.modules["omegaconf"], "OmegaConf", None)
    sys.modules["tqdm"].tqdm = getattr(sys.modules["tqdm"], "tqdm", None)
    sys.modules["torch_ransac3d.plane"].plane_fit = None
    ground = importlib.import_module("src.utils.ground")
    keys = importlib.import_module("src.utils.keys")

    tree = ast.parse(open(os.path.join(REF, "src/transforms/point.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GroundElevation")
    ns = {"torch": torch, "Transform": object, "filter_kwargs": keys.filter_kwargs}
    for name in ground.__all__:
        ns[name] = getattr(ground, name)
    exec(compile(ast.Module(body=[cls], type_ignores=[]), "point.py", "exec"), ns)
    return ground, ns["GroundElevation"]


class DuckData:
    def __init__(self, pos):
        self.pos = pos

    num_points = property(lambda self: self.pos.shape[0])


def make_cloud(rng):
    a0, b0, c0 = 0.03, -0.02, -1.25

    def plane(xy):
        return a0 * xy[:, 0].astype(np.float64) + b0 * xy[:, 1].astype(np.float64) + c0

    def box(n, x0, x1, y0, y1):
        return np.stack((rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)), axis=1).astype(np.float32)

    g = box(3600, -12, 14, -9, 11)
    g = g[~((g[:, 0] > 8) & (g[:, 1] > 5))]                       # the clutter-only corner
    c = box(2300, -12, 14, -9, 11)
    pit = box(60, -3, -2, 2, 3)
    xy = np.concatenate((g, c, pit))
    z = plane(xy)
    z[len(g):len(g) + len(c)] += rng.uniform(0.05, 3.0, len(c))
    z[len(g) + len(c):] -= rng.uniform(0.3, 0.6, len(pit))
    pos = np.concatenate((xy, z.astype(np.float32)[:, None]), axis=1).astype(np.float32)
    is_ground = np.arange(len(pos)) < len(g)
    perm = rng.permutation(len(pos))
    return pos[perm], is_ground[perm]


def unique_cell_minima(pos, grid):
    i, j = R.cell_coords(pos, grid)
    cell = (i - i.min()) * (j.max() - j.min() + 1) + (j - j.min())
    for c in np.unique(cell):
        z = np.sort(pos[cell == c, 2])
        if z.size > 1 and z[0] == z[1]:
            return False
    return True


def draw_samples(rng, trimmed, ground_in_trimmed):
    """NUM_SAMPLES valid triplets, every third one unrestricted (clutter / pit points allowed),
    the others all-ground, each with every residual at least MARGIN away from the threshold."""
    m = trimmed.shape[0]
    ground_ids = np.nonzero(ground_in_trimmed)[0]
    out = []
    while len(out) < NUM_SAMPLES:
        pool = np.arange(m) if len(out) % 3 == 2 else ground_ids
        s = rng.choice(pool, 3, replace=False)
        planes, valid = R.hypothesis_planes(trimmed, s[None])
        if not valid[0]:
            continue
        _, closest = R.score(trimmed, planes, valid)
        if closest > 2 * R.MARGIN:
            out.append(s)
    return np.stack(out)


def main():
    ground, GroundElevation = load_reference()
    rng = np.random.default_rng(20250310)
    pos_np, is_ground = make_cloud(rng)
    assert unique_cell_minima(pos_np, 1.0) and unique_cell_minima(pos_np, 2.0)
    assert pos_np[:, 0].min() < -1 and pos_np[:, 0].max() > 1
    assert pos_np[:, 1].min() < -1 and pos_np[:, 1].max() > 1
    pos = torch.from_numpy(pos_np)
    out = {"pos": pos_np, "is_ground": is_ground.astype(np.uint8)}
    for case in R.CASES:
        prm = R.CASE_PARAMS[case]
        t = GroundElevation(scale=R.SCALE, **prm)
        # each filter on its own, then the transform
        mask = torch.ones(pos.shape[0], dtype=torch.bool)
        if "z_threshold" in prm:
            mz = ground.filter_by_z_distance_of_global_min(pos, prm["z_threshold"])
            out[f"{case}_mask_z"] = mz.numpy()
            mask &= mz
        if "xy_grid" in prm:
            mc = ground.filter_by_local_z_min(pos, prm["xy_grid"])
            out[f"{case}_mask_cell"] = mc.numpy()
            mask &= mc
        index = torch.where(mask)[0].numpy()
        trimmed = pos_np[index]
        # the fitted model, caught where single_plane_model creates it
        caught = []
        inner = ground.RANSACRegressor

        class Catch(inner):
            def fit(self, *a, **k):
                caught.append(self)
                return super().fit(*a, **k)
        ground.RANSACRegressor = Catch
        try:
            data = t._process(DuckData(pos.clone()))
        finally:
            ground.RANSACRegressor = inner
        assert len(caught) == 1
        ransac = caught[0]
        plane = np.array([ransac.estimator_.coef_[0], ransac.estimator_.coef_[1],
                          ransac.estimator_.intercept_], dtype=np.float64)
        inliers = np.asarray(ransac.inlier_mask_)
        assert inliers.shape[0] == index.shape[0]
        assert np.array_equal(inliers, is_ground[index]), \
            f"{case}: the reference's inlier set is not the planar ground of the trimmed set"
        # the clutter-only corner and the pit made it into the trimmed set where a grid is used
        if "xy_grid" in prm:
            assert (~is_ground[index]).sum() >= 5
        samples = draw_samples(rng, trimmed.astype(np.float64), is_ground[index])
        planes, valid = R.hypothesis_planes(trimmed, samples)
        counts, closest = R.score(trimmed, planes, valid)
        assert valid.all() and closest > R.MARGIN, (case, closest)      # EVERY pair
        assert counts.max() == is_ground[index].sum()
        out[f"{case}_index"] = index.astype(np.int32)
        out[f"{case}_plane"] = plane
        out[f"{case}_inliers"] = inliers
        out[f"{case}_elevation"] = data.elevation.numpy()
        out[f"{case}_samples"] = samples.astype(np.int32)
        print(f"{case}: {index.shape[0]} trimmed of {pos.shape[0]}, {int(inliers.sum())} inliers, "
              f"plane {plane.tolist()}, elevation dtype {data.elevation.dtype}, closest residual to "
              f"the threshold {closest:.3e}, counts {np.unique(counts).tolist()[:6]}..")
    mg.save("ground.npz", **out)


if __name__ == "__main__":
    main()
