"""GroundElevation at scene size: ``ground.ground_elevation`` (the kernels of csrc/ground.hip)
against the reference's composition restated in torch on the device (the three filters as
src/utils/ground.py writes them - global min, ``div(..., 'trunc')`` binning, ``unique`` for the
consecutive cell ids, a scatter-min and its argmin, a boolean gather - and the SAME ``H``
hypotheses scored through ``[M, H]`` temporaries, which is what the third-party GPU RANSAC of the
reference's device branch does; the final least-squares fit with ``lstsq``).  The cloud is a
voxelised synthetic scene with a tilted ground slab added below it.

    python tools/ground_bench.py [S|T] [--leg all|new|torch] [--reps N] [--grid G] [--z Z] [--no-grid]

``--leg`` other than ``all`` runs that leg alone, for a kernel trace of its own:
    rocprofv3 --kernel-trace -d <dir> -- python tools/ground_bench.py S --leg new
    python tools/rocpd_summary.py <dir>
``--no-grid`` drops the cell filter: the trimmed set is then of the order of N and the scoring pass
carries the time (the ``[M, H]`` route may not fit in memory at scene S: it is skipped on an
out-of-memory error and reported as such).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import ground  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402

H, THRESHOLD, SCALE, SEED = 100, 1e-3, 4.0, 0


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


def composition(pos, z_threshold, xy_grid, u):
    """The reference's steps in torch; returns (elevation [N, 1], M, best count, plane)."""
    n = pos.shape[0]
    z = pos[:, 2]
    mask = torch.ones(n, dtype=torch.bool, device=pos.device)
    if z_threshold is not None:
        mask = mask & (z - z.min() < z_threshold)
    if xy_grid:
        # divisor as a device tensor: torch's device kernel multiplies by an f32 1 / grid when the
        # divisor is a Python number, which moves points on cell boundaries
        g = torch.tensor(xy_grid, dtype=torch.float32, device=pos.device)
        i = pos[:, 0].div(g, rounding_mode="trunc").long()
        j = pos[:, 1].div(g, rounding_mode="trunc").long()
        i, j = i - i.min(), j - j.min()
        cell = torch.unique(i * (max(i.max(), j.max()) + 1) + j, return_inverse=True)[1]
        num = int(cell.max()) + 1
        zmin = torch.full((num,), float("inf"), device=pos.device).scatter_reduce_(0, cell, z, "amin")
        cand = torch.where(z == zmin[cell])[0]
        arg = torch.full((num,), n, dtype=torch.long, device=pos.device).scatter_reduce_(
            0, cell[cand], cand, "amin")
        low = torch.zeros(n, dtype=torch.bool, device=pos.device)
        low[arg] = True
        mask = mask & low
    t = pos[mask].double()
    m = t.shape[0]
    s = (u.double() * m).floor().long().clamp(max=m - 1)
    p0, p1, p2 = t[s[:, 0]], t[s[:, 1]], t[s[:, 2]]
    d1, d2 = p1 - p0, p2 - p0
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    a = (d1[:, 2] * d2[:, 1] - d2[:, 2] * d1[:, 1]) / det
    b = (d1[:, 0] * d2[:, 2] - d2[:, 0] * d1[:, 2]) / det
    c = p0[:, 2] - (a * p0[:, 0] + b * p0[:, 1])
    r = (t[:, 2:3] - (t[:, 0:1] * a + t[:, 1:2] * b + c)).abs()          # [M, H]
    counts = (r < THRESHOLD).sum(dim=0)
    counts = torch.where(torch.isfinite(a + b + c), counts, torch.full_like(counts, -1))
    best = int(torch.argmax(counts))
    inl = t[r[:, best] < THRESHOLD]
    mean = inl.mean(dim=0)
    sol = torch.linalg.lstsq(inl[:, :2] - mean[:2], (inl[:, 2] - mean[2]).unsqueeze(1)).solution.view(-1)
    plane = (float(sol[0]), float(sol[1]), float(mean[2] - sol[0] * mean[0] - sol[1] * mean[1]))
    pd = pos.double()
    elev = ((pd[:, 2] - (plane[0] * pd[:, 0] + plane[1] * pd[:, 1] + plane[2])) / SCALE).float().view(-1, 1)
    return elev, m, int(counts[best]), plane


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--grid", type=float, default=1.0)
    ap.add_argument("--z", type=float, default=5.0)
    ap.add_argument("--no-grid", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pos = make_voxel_cloud(SCENES[a.scene][0], voxel=0.03, seed=4321, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    lo, hi = pos.min(dim=0).values, pos.max(dim=0).values
    n_ground = pos.shape[0] // 10                                   # a tilted slab under the scene
    g = torch.rand(n_ground, 3, generator=gen, device=dev)
    gxy = lo[:2] + g[:, :2] * (hi[:2] - lo[:2])
    gz = (lo[2] - 2.0 + 0.01 * gxy[:, 0].double() - 0.02 * gxy[:, 1].double()).float()
    pos = torch.cat((pos, torch.cat((gxy, gz.view(-1, 1)), dim=1)))
    pos = pos[torch.randperm(pos.shape[0], generator=gen, device=dev)].contiguous()
    n = pos.shape[0]
    grid = None if a.no_grid else a.grid
    ugen = torch.Generator(device=dev)
    ugen.manual_seed(SEED)
    u = torch.rand(H, 3, generator=ugen, device=dev)                # fit_ground_plane's own draw

    def new():
        return ground.ground_elevation(pos, z_threshold=a.z, xy_grid=grid, scale=SCALE,
                                       num_hypotheses=H, residual_threshold=THRESHOLD,
                                       random_state=SEED)

    def torch_leg():
        return composition(pos, a.z, grid, u)

    legs = {"new": ("ground kernels (bounds, cell min, trim, ransac, elevation)", new),
            "torch": ("torch composition (unique, scatter-min, [M, H] scoring, lstsq)", torch_leg)}
    if a.leg == "all":                                              # (a traced leg runs nothing but itself)
        e, p = new()
        line = (f"scene {a.scene}: {n} points, z_threshold {a.z}, xy_grid {grid}: {p.num_trimmed} trimmed, "
                f"best hypothesis {p.best_index} with {p.best_count} inliers, plane {p.plane}")
        try:
            e2, m2, c2, p2 = torch_leg()
            line += (f"; composition: {m2} trimmed, {c2} inliers, plane {p2}, elevation differs by "
                     f"{float((e - e2).abs().max()):.2e}")
            del e2
        except torch.cuda.OutOfMemoryError:
            line += "; composition: out of memory"
            legs.pop("torch")
        print(line)
        del e
    for key, (name, fn) in legs.items():
        if a.leg in ("all", key):
            med, best, wall = timed(fn, a.reps)
            print(f"{name}: device {med:.3f} ms median / {best:.3f} ms min, "
                  f"host wall {wall:.3f} ms median over {a.reps} calls (+ 2 warm-up calls)")


if __name__ == "__main__":
    main()
