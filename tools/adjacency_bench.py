"""The partition's input graph at scene size: ``graph.partition_adjacency`` (the kernels of
csrc/adjacency.hip) against the reference's composition restated in torch on the device
(AdjacencyGraph -> ConnectIsolated -> to_trimmed through the shims' coalesce: expand the table
to an edge list, masks, unique-style isolated search, sort-based duplicate removal).  The table
is the library's own ``knn_1`` (k = 45, r = 2 m) of a voxelised synthetic cloud plus a few far
outliers, so some nodes are isolated; the graph uses its first 10 columns.

    python tools/adjacency_bench.py [S|T] [--leg all|new|torch] [--reps N] [--order shuffled|spatial]

``--leg`` other than ``all`` runs that leg alone, for a kernel trace of its own:
    rocprofv3 --kernel-trace -d <dir> -- python tools/adjacency_bench.py S --leg new
    python tools/rocpd_summary.py <dir>
``--order spatial`` sorts the cloud along a Morton curve first (partner rows then sit close in
memory); ``shuffled`` is the synthetic cloud's random row order, the worst case for the look-ups.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import graph  # noqa: E402
from superpoint_transformer_amd.neighbors import knn_1  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402
from superpoint_transformer_amd.transforms import morton_code  # noqa: E402

K_TABLE, R_MAX, K, W = 45, 2.0, 10, 1.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", default="shuffled", choices=["shuffled", "spatial"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pos = make_voxel_cloud(SCENES[a.scene][0], voxel=0.03, seed=4321, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    far = torch.rand(64, 3, generator=gen, device=dev) * 40 + 100
    pos = torch.cat((pos, far))
    if a.order == "spatial":
        pos = pos[torch.argsort(morton_code(pos))].contiguous()
    else:
        pos = pos[torch.randperm(pos.shape[0], generator=gen, device=dev)].contiguous()
    nn, dist = knn_1(pos, K_TABLE, r_max=R_MAX)
    n = pos.shape[0]

    def new():
        return graph.partition_adjacency(nn, dist, K, w=W, pos=pos, k_isolated=1, reduce="mean")

    def composition():
        return graph._partition_adjacency_torch(nn, dist, K, W, pos, 1, "mean", None)

    if a.leg == "all":                                          # (a traced leg runs nothing but itself)
        g, r = new(), composition()
        same = torch.equal(g.edge_index, r.edge_index) and torch.equal(g.source_csr, r.source_csr)
        dw = float((g.edge_attr - r.edge_attr).abs().max() / r.edge_attr.abs().max())
        print(f"scene {a.scene} ({a.order} rows): {n} points, table [{n}, {K_TABLE}], k = {K}: "
              f"{int((nn[:, :K] >= 0).sum())} directed entries -> {g.edge_index.shape[1]} edges, "
              f"{g.num_isolated} isolated; indices equal to the composition's: {same}, "
              f"weights differ by {dw:.2e}")
        del g, r
    legs = {"new": ("adjacency kernels (stats, count, fill)", new),
            "torch": ("torch composition (edge list, coalesce sort)", composition)}
    for key, (name, fn) in legs.items():
        if a.leg in ("all", key):
            med, best, wall = timed(fn, a.reps)
            print(f"{name}: device {med:.3f} ms median / {best:.3f} ms min, "
                  f"host wall {wall:.3f} ms median over {a.reps} calls (+ 2 warm-up calls)")


if __name__ == "__main__":
    main()
