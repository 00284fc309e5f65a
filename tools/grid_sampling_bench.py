"""GridSampling3D at scene size: ``transforms.GridSampling3D`` (the kernels of csrc/voxel.hip)
against the reference's composition restated in torch on the same device and the same inputs
(``round``, the restated ``grid_cluster``, a ``torch.unique`` for ``consecutive_cluster`` with its
``scatter_`` of an arange, a second ``unique`` inside ``atomic_to_histogram``, one scatter per key,
a sort for ``sub``), with its host reads counted.  The yardstick is that composition, never the
new code itself.

The raw cloud: ``synthetic.make_voxel_cloud`` at the scene's size, every voxel repeated
``--per-voxel`` times (default 4) with a jitter of +-0.4 voxel, rows shuffled; keys of the default
config: pos, rgb, intensity (f32), y (int64, 14 bins), sub = arange.

    python tools/grid_sampling_bench.py [S|T|R] [--reps N] [--per-voxel K] [--leg all|new|torch]

Per kernel group the table gives the device-time median, the minimum bytes the step has to move
(formulas in ``min_bytes``) and the fraction of 8 TB/s that this makes.
"""
import argparse
import math
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import voxel  # noqa: E402
from superpoint_transformer_amd.data import Data  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402
from superpoint_transformer_amd.transforms import GridSampling3D  # noqa: E402

SIZE, N_BINS, PEAK = 0.03, 14, 8e12


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


def raw_cloud(scene, per_voxel, dev):
    vox = make_voxel_cloud(SCENES[scene][0], voxel=SIZE, seed=4321, device=dev)
    gen = torch.Generator(device=dev).manual_seed(6)
    pos = vox.repeat_interleave(per_voxel, dim=0)
    pos += (torch.rand(pos.shape, generator=gen, device=dev) - 0.5) * (0.8 * SIZE)
    pos = pos[torch.randperm(pos.shape[0], generator=gen, device=dev)].contiguous()
    n = pos.shape[0]
    return dict(pos=pos, rgb=torch.rand(n, 3, generator=gen, device=dev),
                intensity=torch.rand(n, generator=gen, device=dev),
                y=torch.randint(0, N_BINS, (n,), generator=gen, device=dev),
                sub=torch.arange(n, device=dev))


def composition(f):
    """The reference's steps in torch on the device; returns the grouped keys."""
    pos, dev = f["pos"], f["pos"].device
    n = pos.shape[0]
    coords = torch.round(pos / SIZE)
    start, end = coords.min(dim=0).values, coords.max(dim=0).values
    c = (coords - start).long()
    num = (end - start).long() + 1
    cluster = c[:, 0] + c[:, 1] * num[0] + c[:, 2] * (num[0] * num[1])
    uniq, inv = torch.unique(cluster, sorted=True, return_inverse=True)          # consecutive_cluster
    v = uniq.numel()
    perm = inv.new_empty(v).scatter_(0, inv, torch.arange(n, device=dev))        # duplicates: unspecified
    count = torch.bincount(inv, minlength=v).clamp(min=1)
    out = {"perm": perm}
    for k in ("pos", "rgb", "intensity"):                                        # scatter_mean per key
        x = f[k]
        s = torch.zeros((v,) + tuple(x.shape[1:]), device=dev).index_add_(0, inv, x)
        out[k] = s / count.view((-1,) + (1,) * (x.dim() - 1)).float()
    y = f["y"]
    assert bool(y.ge(0).all())                                                   # atomic_to_histogram
    rows = int(inv.max()) + 1
    hist_idx = N_BINS * inv + y
    u2, inv2 = torch.unique(hist_idx, sorted=True, return_inverse=True)
    perm2 = inv2.new_empty(u2.numel()).scatter_(0, inv2, torch.arange(n, device=dev))
    counts = torch.bincount(inv2)
    hist = torch.zeros((rows, N_BINS), dtype=torch.long, device=dev)
    hist[hist_idx[perm2] // N_BINS, hist_idx[perm2] % N_BINS] = counts
    out["y"] = hist
    sorted_idx, order = inv.sort()                                               # Cluster(dense=True)
    heads = torch.where(sorted_idx[1:] > sorted_idx[:-1])[0] + 1
    out["sub"] = (torch.cat([heads.new_zeros(1), heads, heads.new_full((1,), n)]), f["sub"][order])
    return out


def host_reads(fn):
    """Synchronising calls of one run, counted through torch's sync debug mode."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
        return sum("synchroniz" in str(x.message) for x in w)
    except Exception:
        return -1
    finally:
        torch.cuda.set_sync_debug_mode("default")


def min_bytes(n, v, key_bits):
    """Bytes each step has to move at the least (n points, v voxels)."""
    passes = math.ceil(min(key_bits, 32) / 8) + (math.ceil((key_bits - 32) / 8) if key_bits > 32 else 0)
    words = 2 if key_bits > 32 else 1
    return {
        "bounds": 12 * n,
        # keys: pos in, key words out; a pass: 4n (digit histogram) + 8n in + 8n out; heads + scan:
        # 4n in, 4(n+1) x 3; groups: 16n in, order + cluster 16n out, 28 v out
        "groups": 12 * n + 4 * words * n + passes * 20 * n + 16 * n + 32 * n + 28 * v,
        "mean pos": 8 * n + 8 * v + 12 * n + 12 * v,
        "mean rgb": 8 * n + 8 * v + 12 * n + 12 * v,
        "mean intensity": 8 * n + 8 * v + 4 * n + 4 * v,
        "histogram y": 8 * n + 8 * v + 8 * n + 8 * N_BINS * v,
        "sub gather": 8 * n + 8 * n + 8 * n,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-voxel", type=int, default=4)
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    f = raw_cloud(a.scene, a.per_voxel, dev)
    n = f["pos"].shape[0]
    # inplace like the default config: the Data built per call is rebound key by key, `f` is not touched
    t = GridSampling3D(SIZE, hist_key="y", hist_size=N_BINS, inplace=True)

    def new():
        return t(Data(**f))

    def torch_leg():
        return composition(f)

    out = new()
    g = t.groups_
    v = g.num_voxels
    c = g.coords
    key_bits = sum(int(x).bit_length() for x in (c.max(dim=0).values - c.min(dim=0).values).tolist())
    print(f"scene {a.scene}: {n} raw points -> {v} voxels ({n / v:.2f} per voxel), key {key_bits} bits")
    if a.leg == "all":
        ref = torch_leg()
        same = {k: bool(torch.equal(out[k], ref[k])) for k in ("pos", "rgb", "intensity", "y")}
        same["sub pointers"] = bool(torch.equal(out.sub.pointers, ref["sub"][0]))
        print(f"bit-equal to the composition (float atomics there: not expected for means): {same}")
        del ref
    legs = {"new": ("GridSampling3D (csrc/voxel.hip)", new),
            "torch": ("torch composition of the reference's steps", torch_leg)}
    for key, (name, fn) in legs.items():
        if a.leg in ("all", key):
            med, best, wall = timed(fn, a.reps)
            print(f"{name}: device {med:.2f} ms median / {best:.2f} ms min, host wall {wall:.2f} ms "
                  f"median over {a.reps} calls (+ 2 warm-up calls), host reads {host_reads(fn)}")
    if a.leg in ("all", "new"):
        steps = {
            "groups": lambda: voxel.voxel_groups(f["pos"], SIZE),          # bounds + groups + 2 host reads
            "mean pos": lambda: voxel.group_mean(f["pos"], g),
            "mean rgb": lambda: voxel.group_mean(f["rgb"], g),
            "mean intensity": lambda: voxel.group_mean(f["intensity"], g),
            "histogram y": lambda: voxel.group_histogram(f["y"], g, N_BINS),
            "sub gather": lambda: f["sub"][g.order],
        }
        mb = min_bytes(n, v, key_bits)
        mb["groups"] += mb.pop("bounds")
        print(f"{'step':<16}{'ms median':>12}{'min MB':>12}{'of 8 TB/s':>12}")
        for name, fn in steps.items():
            med, _, _ = timed(fn, a.reps)
            print(f"{name:<16}{med:>12.3f}{mb[name] / 1e6:>12.1f}{mb[name] / (med * 1e-3) / PEAK:>11.1%}")


if __name__ == "__main__":
    main()
