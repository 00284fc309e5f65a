"""PointFeatures at scene size: ``features.point_colors`` (rgb + hsv + lab in one pass),
``features.point_density`` and the fused ``features.partition_input`` (the kernels of
csrc/point_feat.hip) against the reference's composition restated in torch on the device:
``to_float_rgb`` with its host read of the max, ``rgb2hsv`` with its stack / gather, ``rgb2lab``
with its boolean-mask assignments, 3x3 matmuls and ``round(decimals=4)``, the three-pass density,
and ``torch.cat`` for ``AddKeysTo``.  The cloud is a voxelised synthetic scene with random uint8
colours and the library's own ``knn_1`` table.

    python tools/point_features_bench.py [S|T] [--k 45] [--leg all|new|torch] [--reps N]

Achieved GB/s are against the bytes each step has to move: colours 3 B in + 36 B out per point,
density 12 k B in + 4 B out per point.  ``--leg`` other than ``all`` runs that leg alone, for a
kernel trace of its own:
    rocprofv3 --kernel-trace -d <dir> -- python tools/point_features_bench.py S --leg new
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import features  # noqa: E402
from superpoint_transformer_amd.data import Data  # noqa: E402
from superpoint_transformer_amd.neighbors import knn_1  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402

PARTITION_KEYS = ["rgb", "linearity", "planarity", "scattering", "verticality", "elevation"]
POINT_KEYS = PARTITION_KEYS + ["density", "hsv", "lab"]


def timed(fn, reps, settle=0.3):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    time.sleep(settle)
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
    ev.sort(), wall.sort()
    return ev[len(ev) // 2], ev[0], wall[len(wall) // 2]


def to_float_rgb(rgb):
    rgb = rgb.float()
    if rgb.max() > 1:                                   # host read
        rgb = rgb / 255
    return rgb.clamp(min=0, max=1)


def torch_hsv(rgb):
    rgb = to_float_rgb(rgb.clone())
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    mx = rgb.max(1).values
    mn, arg = rgb.min(1)
    mm = mx - mn + 1e-10
    h1 = 60.0 * (g - r) / mm + 60.0
    h2 = 60.0 * (b - g) / mm + 180.0
    h3 = 60.0 * (r - b) / mm + 300.0
    h = torch.stack((h2, h3, h1), dim=0).gather(dim=0, index=arg.unsqueeze(0)).squeeze(0)
    out = torch.stack((h, mm / (mx + 1e-10), mx), dim=1)
    out[:, 0] /= 360.
    return out


def torch_lab(rgb):
    dev = rgb.device
    rgb = to_float_rgb(rgb.clone())
    mask = rgb > 0.04045
    rgb[mask] = ((rgb[mask] + 0.055) / 1.055) ** 2.4
    rgb[~mask] = rgb[~mask] / 12.92
    rgb *= 100
    m = torch.tensor([[0.4124, 0.2126, 0.0193], [0.3576, 0.7152, 0.1192],
                      [0.1805, 0.0722, 0.9505]], device=dev)
    xyz = (rgb @ m).round(decimals=4)
    xyz /= torch.tensor([[95.047, 100.0, 108.883]], device=dev)
    mask = xyz > 0.008856
    xyz[mask] = xyz[mask] ** (1 / 3.)
    xyz[~mask] = 7.787 * xyz[~mask] + 1 / 7.25
    m = torch.tensor([[0, 500, 0], [116, -500, 200], [0, 0, -200]], device=dev, dtype=torch.float)
    lab = xyz @ m
    lab[:, 0] -= 16
    return lab.round(decimals=4) / 100


def torch_colors(rgb):
    return {"rgb": to_float_rgb(rgb), "hsv": torch_hsv(to_float_rgb(rgb)),
            "lab": torch_lab(to_float_rgb(rgb))}


def torch_density(nn, dist):
    dmax = dist.max(dim=1).values
    k = nn.ge(0).sum(dim=1)
    return (k / dmax ** 2).view(-1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--k", type=int, default=45)
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pos = make_voxel_cloud(SCENES[a.scene][0], voxel=0.03, seed=4321, device=dev).contiguous()
    n, k = pos.shape[0], a.k
    gen = torch.Generator(device=dev).manual_seed(5)
    rgb = torch.randint(0, 256, (n, 3), generator=gen, device=dev, dtype=torch.uint8)
    elevation = torch.rand(n, 1, generator=gen, device=dev)
    nn, dist = knn_1(pos, k, r_max=2.0)
    torch.cuda.synchronize()
    color_bytes, density_bytes = n * (3 + 36), n * (12 * k + 4)
    print(f"scene {a.scene}: {n} points, k = {k}; colours move {color_bytes / 1e9:.3f} GB, "
          f"density {density_bytes / 1e9:.3f} GB")

    def data():
        return Data(pos=pos, rgb=rgb, neighbor_index=nn, neighbor_distance=dist,
                    elevation=elevation)

    def two_steps():
        d = features.point_features(data(), POINT_KEYS)
        d.add_keys_to(PARTITION_KEYS, to="x", delete_after=False)
        return d

    def torch_two_steps():
        d = data()
        for key, v in torch_colors(rgb).items():
            d[key] = v
        d.density = torch_density(nn, dist)
        d.add_keys_to(["rgb", "hsv", "lab", "density", "elevation"], to="x", delete_after=False)
        return d

    legs = [
        ("new", "point_colors rgb + hsv + lab", lambda: features.point_colors(rgb), color_bytes),
        ("torch", "torch composition of the colours", lambda: torch_colors(rgb), color_bytes),
        ("new", "point_density", lambda: features.point_density(nn, dist), density_bytes),
        ("torch", "torch composition of the density", lambda: torch_density(nn, dist),
         density_bytes),
        ("new", "partition_input (colours, density, eigenfeatures, x)",
         lambda: features.partition_input(data(), POINT_KEYS, PARTITION_KEYS), None),
        ("new", "PointFeatures + AddKeysTo (same keys, two steps)", two_steps, None),
        ("torch", "torch colours + density + cat (no eigenfeatures)", torch_two_steps, None),
    ]
    if a.leg == "all":
        new, ref = features.point_colors(rgb), torch_colors(rgb)
        line = "kernel vs torch composition on the device, max abs difference:"
        for key in ("rgb", "hsv", "lab"):
            line += f" {key} {float((new[key] - ref[key]).abs().max()):.2e}"
        d = (features.point_density(nn, dist) - torch_density(nn, dist)).abs()
        print(line + f" density {float(d[torch.isfinite(d)].max()):.2e}")
        del new, ref, d
    for leg, name, fn, nbytes in legs:
        if a.leg not in ("all", leg):
            continue
        try:
            med, best, wall = timed(fn, a.reps)
        except torch.cuda.OutOfMemoryError:
            print(f"{name}: out of memory")
            continue
        rate = f", {nbytes / med / 1e6:.0f} GB/s at the median" if nbytes else ""
        print(f"{name}: device {med:.3f} ms median / {best:.3f} ms min, host wall {wall:.3f} ms "
              f"median over {a.reps} calls (+ 2 warm-up calls){rate}")


if __name__ == "__main__":
    main()
