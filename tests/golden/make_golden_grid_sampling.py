"""Golden fixture for ``GridSampling3D``, produced by the REFERENCE'S OWN
``GridSampling3D.__init__`` / ``_process`` and ``_group_data`` (src/transforms/sampling.py:86-468;
the class and the function are cut out of the file with ``ast`` - unmodified - because the module
pulls torch_cluster, torch_geometric and the whole ``src.data`` package at import), the
verbatim-imported ``src/utils/histogram.py`` (``atomic_to_histogram``), ``src/utils/tensor.py``
(``cast_to_optimal_integer_type``), ``src/utils/keys.py`` (``sanitize_keys``) and the reference's
``InstanceData`` / ``Cluster`` (src/data/instance.py, cluster.py, csr.py, loaded as
make_golden_instance.py does).

Stand-ins: ``grid_cluster`` / ``voxel_grid`` are the restatements of tests/grid_sampling_reference.py
("[third-party restated]": torch_cluster and torch_geometric are not installed here, so they cannot
be pinned), ``consecutive_cluster`` / ``scatter_mean`` / ``scatter_sum`` those of
oracle/spt_oracle.py (run on ONE thread: see ``build``), ``Shuffle`` the identity
(``mode='last'`` then keeps the highest index of every voxel) and the ``Data`` a duck-typed
attribute store.

The cloud (about 3 500 points, voxel size 0.25, coordinates on both sides of the origin):
  * a box of scattered points, most voxels with 1 - 4 of them;
  * one voxel with 320 points whose values sit on an offset, so that the reference's f32 mean has
    a rounding error worth measuring;
  * 400 points on a sparse lattice, each its own voxel;
  * a block placed exactly on half-way values (+-0.125, +-0.375, ...): ``round`` ties to even;
  * keys in stored order: pos, rgb, intensity, normal (f32), obj (int64, in front of y), y (int64
    in [0, 14)), is_val (bool), sub (arange), other (a tensor of another length, left alone).
Cases: tests/grid_sampling_reference.py ``CASES``.  The script asserts that the restatement
reproduces every stored array bit for bit and prints the reference's own f32 deviation from the
f64 restatement.

Usage (build container only): python tests/golden/make_golden_grid_sampling.py [--check]
(``--check``: regenerate and compare with the committed file array by array, bit for bit).
"""
import ast
import copy
import importlib
import math
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_select as mgs  # noqa: E402
import make_golden_instance as mgi  # noqa: E402
import grid_sampling_reference as R  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

REF = mg.REF


class IdentityShuffle:
    def __call__(self, data):
        return data


def load_reference():
    U, csr, inst = mgi.load_reference()
    cluster = sys.modules["src.data.cluster"]
    hist = importlib.import_module("src.utils.histogram")
    keys = importlib.import_module("src.utils.keys")
    tensor = importlib.import_module("src.utils.tensor")
    tree = ast.parse(open(os.path.join(REF, "src/transforms/sampling.py")).read())

    def node(kind, name):
        return next(n for n in tree.body if isinstance(n, kind) and n.name == name)

    ns = {"torch": torch, "re": re, "math": math, "Transform": object,
          "Shuffle": IdentityShuffle, "grid_cluster": R.grid_cluster, "voxel_grid": R.voxel_grid,
          "cast_to_optimal_integer_type": tensor.cast_to_optimal_integer_type,
          "consecutive_cluster": O.consecutive_cluster, "sanitize_keys": keys.sanitize_keys,
          "InstanceData": inst.InstanceData, "Cluster": cluster.Cluster, "CSRData": csr.CSRData,
          "atomic_to_histogram": hist.atomic_to_histogram, "scatter_mean": O.scatter_mean,
          "split_histogram": hist.split_histogram, "Batch": None}
    body = [node(ast.ClassDef, "SaveNodeIndex"), node(ast.ClassDef, "GridSampling3D"),
            node(ast.FunctionDef, "_group_data")]
    exec(compile(ast.Module(body=body, type_ignores=[]), "sampling.py", "exec"), ns)
    return ns["GridSampling3D"], ns["SaveNodeIndex"]


class DuckData(mgs.DuckData):
    def __contains__(self, k):
        return k in self._s

    num_points = property(lambda self: self.pos.shape[0])

    def clone(self):
        return copy.deepcopy(self)


def make_cloud(rng):
    def f32(a):
        return np.asarray(a, dtype=np.float32)

    box = f32(rng.uniform([-3.0, -2.5, -1.0], [3.0, 2.5, 1.5], (2400, 3)))
    blob = f32(rng.uniform(0.40, 0.60, (320, 3)))                       # voxel (2, 2, 2)
    i = np.arange(400)
    lattice = f32(np.stack((4.0 + (i % 20) * 0.5, -6.0 - (i // 20) * 0.5,
                            2.0 + rng.uniform(-0.1, 0.1, 400)), axis=1))
    half = f32(rng.integers(-8, 8, (380, 3)) * 0.25 + 0.125)            # exactly half-way
    half[:, 0] -= 7.0                                                   # a block of its own
    assert np.all(np.abs(half / np.float32(0.25) % 1.0) == 0.5)
    pos = np.concatenate((box, blob, lattice, half))
    n = pos.shape[0]
    is_blob = np.zeros(n, dtype=bool)
    is_blob[len(box):len(box) + len(blob)] = True
    rgb = f32(rng.uniform(0, 1, (n, 3)))
    intensity = f32(rng.uniform(0, 1, n))
    # the big voxel's values sit on an offset: a long f32 sum of them rounds visibly
    rgb[is_blob] = f32(0.7 + rng.uniform(0, 0.3, (320, 3)))
    intensity[is_blob] = f32(900.0 + rng.uniform(0, 50, 320))
    normal = rng.normal(size=(n, 3))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.2
    normal = f32(normal / np.linalg.norm(normal, axis=1, keepdims=True))
    y = rng.integers(0, R.NUM_BINS, n).astype(np.int64)
    cell = np.floor(pos / 1.0).astype(np.int64)
    obj = ((cell[:, 0] * 7 + cell[:, 1] * 3 + cell[:, 2]) % 37 + 37) % 37
    obj = np.where(rng.uniform(size=n) < 0.2, rng.integers(0, 37, n), obj).astype(np.int64)
    is_val = rng.uniform(size=n) < 0.45
    batch = rng.integers(0, 3, n).astype(np.int64)
    perm = rng.permutation(n)
    fields = dict(pos=pos[perm], rgb=rgb[perm], intensity=intensity[perm], normal=normal[perm],
                  obj=obj[perm], y=y[perm], is_val=is_val[perm], sub=np.arange(n, dtype=np.int64),
                  other=f32(rng.uniform(size=7)))
    return fields, batch[perm], is_blob[perm]


def run_reference(GridSampling3D, fields, kwargs):
    data = DuckData(**{k: v.clone() for k, v in fields.items()})
    out = GridSampling3D(**kwargs)._process(data)
    res = {}
    for k, v in out:
        if type(v).__name__ == "Cluster":
            res[k] = (v.pointers, v.points)
        elif type(v).__name__ == "InstanceData":
            res[k] = (v.pointers, v.obj, v.count, v.y)
        else:
            res[k] = v
    return res


def build():
    # one thread: torch's CPU index_put_ with duplicate indices (PyG's consecutive_cluster) keeps
    # the LAST writer only then; with several threads the winner changes from run to run
    torch.set_num_threads(1)
    GridSampling3D, _ = load_reference()
    rng = np.random.default_rng(20250615)
    fields_np, batch_np, is_blob = make_cloud(rng)
    fields = {k: torch.from_numpy(v) for k, v in fields_np.items()}
    assert tuple(fields) == R.INPUT_KEYS
    pos = fields["pos"]
    assert float(pos.min()) < -1 and float(pos.max()) > 1
    assert int(fields["y"].max()) < R.NUM_BINS

    out = {f"in__{k}": v for k, v in fields_np.items()}
    out["in__batch"] = batch_np
    worst = {}
    for case, (kwargs, with_batch) in R.CASES.items():
        f = dict(fields)
        if with_batch:
            f["batch"] = torch.from_numpy(batch_np)
        ref = run_reference(GridSampling3D, f, kwargs)
        flat = R.flatten(ref, case, R.CASE_KEYS[case])
        # the restatement reproduces the reference bit for bit, and its two voxel numberings agree
        mine = R.grid_sampling(f, **kwargs)
        for k, v in R.flatten(mine, case, R.CASE_KEYS[case]).items():
            want = flat[k]
            if k.endswith("__sub__points"):       # (the reference's unstable sort: canonical_sub)
                want = R.canonical_sub(flat[k.replace("points", "pointers")], want).numpy()
            assert R.bits_equal(want, v), f"restatement differs from the reference: {k}"
        assert set(flat) == set(R.flatten(mine, case, R.CASE_KEYS[case]))
        coords = torch.round(pos / kwargs["size"])
        assert torch.equal(mine["_cluster"],
                           R.lexicographic_cluster(coords, f.get("batch")))
        counts = torch.bincount(mine["_cluster"])
        if case == "default":
            assert int(counts.max()) >= 300 and int((counts == 1).sum()) >= 400
            blob_voxels = mine["_cluster"][torch.from_numpy(is_blob)].unique()
            assert blob_voxels.numel() == 1 and int(counts[blob_voxels]) >= 320
        if case == "batch":
            key = torch.cat([coords, f["batch"].view(-1, 1).float()], dim=1)
            assert key.unique(dim=0).shape[0] == counts.numel() > coords.unique(dim=0).shape[0]
        m64 = R.grid_sampling(f, dtype=torch.float64, **kwargs)
        for k in R.MEAN_KEYS:
            if f"{case}__{k}" in flat and kwargs.get("mode", "mean") == "mean":
                dev = R.relative_deviation(flat[f"{case}__{k}"], m64[k].numpy())
                worst[k] = max(worst.get(k, 0.0), dev)
        print(f"{case}: {counts.numel()} voxels of {pos.shape[0]} points, largest {int(counts.max())}, "
              f"singles {int((counts == 1).sum())}")
        out.update(flat)
    print("reference f32 deviation from the f64 restatement, max |diff| / max |f64|, worst case:")
    for k, v in worst.items():
        print(f"  {k}: {v:.3e}")
    return out


def main():
    out = build()
    path = os.path.join(HERE, "grid_sampling.npz")
    if "--check" in sys.argv:
        old = dict(np.load(path))
        assert set(old) == set(out), sorted(set(old) ^ set(out))
        for k, v in out.items():
            v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            assert R.bits_equal(old[k], v), f"{k} differs from the committed fixture"
        print(f"grid_sampling.npz: {len(out)} arrays bit-identical to the regenerated ones")
        return
    mg.save("grid_sampling.npz", **out)
    print(f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
