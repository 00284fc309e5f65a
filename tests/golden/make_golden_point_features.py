"""Golden fixture for ``PointFeatures`` (colour keys, density) and ``Data.add_keys_to``, produced
by the REFERENCE'S OWN code: ``to_float_rgb`` (src/utils/color.py:17-22), ``rgb2hsv`` /
``rgb2lab`` (src/utils/features.py:8-86), the ``PointFeatures`` class (src/transforms/point.py:
41-182) and the ``add_keys_to`` method (src/data/data.py:1097-1141), each cut out of its file
with ``ast`` - unmodified - because the modules import plotly / colorhash / the model zoo / PyG.
``sanitize_keys`` and the key lists come from the verbatim-imported src/utils/keys.py.  They run
on the CPU; only inputs and outputs are stored (tests/golden/point_features.npz).

Colour sets (every output through ``PointFeatures(keys=['rgb', 'hsv', 'lab'])._process``):
  * ``u8``: the grey axis and the three primary axes (256 levels each), every two-channel tie
    pattern (a, a, b) / (a, b, a) / (b, a, a) over a 16 x 16 grid of levels, black, white, the
    levels 10 / 11 around the 0.04045 threshold in every combination, a dark cube straddling
    the 0.008856 threshold (asserted below), random colours;
  * ``u8_small``: an integer image of 0 / 1 only: max <= 1, NOT divided by 255;
  * ``f32``: floats in [0, 1] with maximum exactly 1.0 (no division), random rows with
    max - min >= 1 / 64 (asserted: below that the hue is a quotient of two roundings);
  * ``f32_gt1``: floats in [0, 255] (divided by 255), same condition after the division.
Also ``*_direct_*``: ``rgb2hsv`` / ``rgb2lab`` called directly on the ``u8`` set, asserted equal
to what the class stores up to its / 360 and / 100.

Density: a [2000, 13] kNN table pair whose ``[:, 1:]`` slice is the [2000, 12] table the class
sees: full rows, partial rows (-1 padded, distance -1), empty rows, a row of zero distances.

``add_keys_to``: the scenarios of tests/point_features_reference.py on a 7-node duck Data.

Usage (build container only): python tests/golden/make_golden_point_features.py
"""
import ast
import importlib
import os
import sys
from typing import List

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import point_features_reference as R  # noqa: E402

REF = mg.REF


def cut(path, names, ns):
    """exec the top-level definitions ``names`` of a reference file, unmodified, in ``ns``."""
    tree = ast.parse(open(os.path.join(REF, path)).read())
    body = [n for n in tree.body
            if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), os.path.basename(path), "exec"), ns)


def load_reference():
    mg.install_reference_import_hooks()
    keys = importlib.import_module("src.utils.keys")
    ns = {"torch": torch, "np": np, "Transform": object, "List": List,
          "POINT_FEATURES": keys.POINT_FEATURES, "GEOMETRIC_FEATURES": keys.GEOMETRIC_FEATURES,
          "sanitize_keys": keys.sanitize_keys, "geometric_features": None}
    cut("src/utils/color.py", ["to_float_rgb"], ns)
    cut("src/utils/features.py", ["rgb2hsv", "rgb2lab"], ns)
    cut("src/transforms/point.py", ["PointFeatures"], ns)
    # the method: the class body of Data holds it as a FunctionDef
    tree = ast.parse(open(os.path.join(REF, "src/data/data.py")).read())
    data_cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Data")
    fn = next(n for n in data_cls.body
              if isinstance(n, ast.FunctionDef) and n.name == "add_keys_to")
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "data.py", "exec"), ns)
    return ns


class DuckData:
    """What ``PointFeatures._process`` and ``add_keys_to`` touch of a Data."""

    def __init__(self, num_nodes, **attrs):
        self.__dict__["_n"] = num_nodes
        for k, v in attrs.items():
            setattr(self, k, v)

    num_nodes = property(lambda self: self._n)
    keys = property(lambda self: [k for k in self.__dict__ if k != "_n"])
    has_neighbors = property(lambda self: "neighbor_index" in self.__dict__)

    def __getattr__(self, key):                     # absent optional attributes read as None
        if key in ("rgb", "pos", "x", "neighbor_index"):
            return None
        raise AttributeError(key)

    def __setitem__(self, key, value):
        setattr(self, key, value)


def u8_colors(rng):
    lv = np.arange(256)
    z = np.zeros(256, dtype=np.int64)
    parts = [np.stack((lv, lv, lv), 1), np.stack((lv, z, z), 1), np.stack((z, lv, z), 1),
             np.stack((z, z, lv), 1)]
    grid = np.array([0, 1, 5, 10, 11, 17, 40, 64, 99, 127, 128, 170, 200, 254, 255, 33])
    a, b = [v.reshape(-1) for v in np.meshgrid(grid, grid, indexing="ij")]
    parts += [np.stack((a, a, b), 1), np.stack((a, b, a), 1), np.stack((b, a, a), 1)]
    parts.append(np.array([[0, 0, 0], [255, 255, 255], [5, 5, 9], [9, 5, 5], [5, 9, 5]]))
    t = np.array([10, 11])
    parts.append(np.stack([v.reshape(-1) for v in np.meshgrid(t, t, t, indexing="ij")], 1))
    parts.append(np.stack([v.reshape(-1) for v in np.meshgrid(t, [0, 255], t, indexing="ij")], 1))
    d = np.arange(0, 44, 4)
    parts.append(np.stack([v.reshape(-1) for v in np.meshgrid(d, d, d, indexing="ij")], 1))
    fixed = np.concatenate(parts)
    rand = rng.integers(0, 256, (12000 - fixed.shape[0], 3))
    return np.concatenate((fixed, rand)).astype(np.uint8)


def spread_rows(rng, n, scale):
    """n random rows in [0, scale] with (max - min) / scale >= 1 / 64."""
    out = np.empty((0, 3), dtype=np.float32)
    while out.shape[0] < n:
        c = (rng.random((2 * n, 3)) * scale).astype(np.float32)
        c01 = R.to_float_rgb(c) if scale > 1 else c
        out = np.concatenate((out, c[c01.max(1) - c01.min(1) >= 1 / 64]))
    return out[:n]


def knn_tables(rng):
    n, kw = 2000, 13
    idx = rng.integers(0, n, (n, kw)).astype(np.int64)
    dist = np.sort(rng.random((n, kw)).astype(np.float32) * 0.3 + 1e-3, axis=1)
    valid = np.full(n, kw - 1)
    valid[500:1500] = rng.integers(1, kw - 1, 1000)              # partial rows
    valid[1500:1600] = 0                                         # empty rows
    pad = np.arange(kw - 1)[None, :] >= valid[:, None]
    idx[:, 1:][pad] = -1
    dist[:, 1:][pad] = -1.0
    dist[1700, :] = 0.0                                          # zero distances: inf
    dist[1701, 1:] = 0.0
    perm = rng.permutation(n)
    return idx[perm], dist[perm]


def main():
    ns = load_reference()
    PointFeatures = ns["PointFeatures"]
    rng = np.random.default_rng(20250411)
    out = {}

    f32 = spread_rows(rng, 4000, 1.0)
    f32[0] = [1.0, 0.5, 0.25]
    gt1 = spread_rows(rng, 512, 255.0)
    sets = {"u8": u8_colors(rng), "u8_small": rng.integers(0, 2, (64, 3)).astype(np.uint8),
            "f32": f32, "f32_gt1": gt1}
    assert f32.max() == 1.0 and gt1.max() > 1.0 and sets["u8_small"].max() == 1
    for name, rgb in sets.items():
        assert rgb.dtype == R.COLOR_SETS[name]
        data = DuckData(rgb.shape[0], rgb=torch.from_numpy(rgb.copy()))
        PointFeatures(keys=["rgb", "hsv", "lab"])._process(data)
        out[f"{name}_in"] = rgb
        for key in R.COLOR_KEYS:
            v = getattr(data, key)
            assert v.dtype == torch.float32 and tuple(v.shape) == rgb.shape, (name, key)
            out[f"{name}_{key}"] = v.numpy()
        mine = R.colors(rgb)
        assert np.array_equal(mine["rgb"], out[f"{name}_rgb"]), name
        print(name, rgb.shape, "hsv dev", R.relative_deviation(out[f"{name}_hsv"], mine["hsv"]),
              "lab dev", R.relative_deviation(out[f"{name}_lab"], mine["lab"]))
    # both branches of both thresholds are exercised by the uint8 set
    c = R.to_float_rgb(sets["u8"])
    t = R.xyz_over_white(c)
    assert ((c > 0.03) & (c <= 0.04045)).any() and ((c > 0.04045) & (c < 0.05)).any()
    assert ((t > 0.007) & (t <= 0.008856)).any() and ((t > 0.008856) & (t < 0.011)).any()
    # the functions called directly agree with what the class stores
    u8 = torch.from_numpy(sets["u8"].copy())
    direct_hsv = ns["rgb2hsv"](u8)
    direct_hsv[:, 0] /= 360.
    assert torch.equal(direct_hsv, torch.from_numpy(out["u8_hsv"]))
    assert torch.equal(ns["rgb2lab"](u8) / 100, torch.from_numpy(out["u8_lab"]))

    # default keys and overwrite=False on a Data that already holds hsv
    assert PointFeatures().keys == tuple(sorted(set(ns["POINT_FEATURES"])))
    out["default_keys"] = np.array(PointFeatures().keys)
    kept = torch.full((64, 3), 0.25)
    data = DuckData(64, rgb=torch.from_numpy(sets["u8_small"].copy()), hsv=kept.clone())
    PointFeatures(keys=["rgb", "hsv", "lab"], overwrite=False)._process(data)
    assert torch.equal(data.hsv, kept) and data.rgb.dtype == torch.float32

    idx13, dist13 = knn_tables(rng)
    data = DuckData(idx13.shape[0], neighbor_index=torch.from_numpy(idx13)[:, 1:],
                    neighbor_distance=torch.from_numpy(dist13)[:, 1:])
    PointFeatures(keys=["density"])._process(data)
    dens = data.density.numpy()
    assert dens.dtype == np.float32 and dens.shape == (2000, 1)
    assert np.isinf(dens).sum() == 2 and (dens == 0).sum() == 100
    assert np.array_equal(dens, R.density(idx13[:, 1:], dist13[:, 1:]))
    out.update(knn_index13=idx13, knn_distance13=dist13, density=dens)

    add_keys_to = ns["add_keys_to"]
    feats = R.add_keys_inputs()

    def duck(case):
        d = DuckData(7, **{k: torch.from_numpy(v.copy()) for k, v in feats.items() if k != "x0"})
        if case["with_x"]:
            d.x = torch.from_numpy(feats["x0"].copy())
        return d

    for name, case in R.ADD_KEYS_CASES.items():
        d = duck(case)
        add_keys_to(d, keys=case["keys"], to=case["to"], strict=case["strict"],
                    delete_after=case["delete_after"])
        out[f"addkeys_{name}_out"] = getattr(d, case["to"]).numpy()
        out[f"addkeys_{name}_left"] = np.array(sorted(d.keys))
    for name, case in R.ADD_KEYS_ERRORS.items():
        try:
            add_keys_to(duck(case), keys=case["keys"], to=case["to"], strict=case["strict"],
                        delete_after=case["delete_after"])
            raise AssertionError(f"{name}: the reference did not raise")
        except Exception as e:                      # noqa: BLE001 - the reference raises Exception
            assert not isinstance(e, AssertionError), e
            out[f"addkeys_{name}_message"] = np.array(str(e))
    mg.save("point_features.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "point_features.npz"))
    assert size < 900 * 1024, size
    print("point_features.npz:", size, "bytes")


if __name__ == "__main__":
    main()
