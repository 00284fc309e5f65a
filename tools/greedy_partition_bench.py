"""The greedy contour-prior partition at batch and scene size: the device route (the kernels of
csrc/merge.hip) against the package's own torch composition of the same rounds run on device
tensors (``route='torch'``: sorts, gathers, scatter-min and loops over the positions of a run).

The graph is the directed k = 8 nearest-neighbour graph (``knn_1``) of a voxelised synthetic
cloud, D = 7 feature columns (the position's height band and six noisy plateau columns),
``reg = 2e-2``, ``min_size = [5, 30, 90]``: the three levels of ``GreedyContourPriorPartition``,
each timed on its own, then the rounds of level 0 one by one.

    python tools/greedy_partition_bench.py [T|S] [--leg all|new|torch] [--reps N] [--levels L]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import partition as P  # noqa: E402
from superpoint_transformer_amd.data import Data  # noqa: E402
from superpoint_transformer_amd.neighbors import knn_1  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402

K, D, REG, MIN_SIZE = 8, 7, 2e-2, [5, 30, 90]


def timed(fn, reps):
    """(median device ms, median host wall ms, peak bytes allocated) over ``reps`` calls after one
    warm-up call."""
    fn()
    torch.cuda.synchronize()
    ev, wall, peak = [], [], 0
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
        peak = max(peak, torch.cuda.max_memory_allocated())
    ev.sort(), wall.sort()
    return ev[len(ev) // 2], wall[len(wall) // 2], peak


def features(pos, gen):
    """[N, 7] f32: six columns of 4 m plateaus in x / y with noise 0.3, the height in metres."""
    cell = torch.floor(pos[:, :2] / 4.0)
    cols = [((cell[:, i % 2] * (3 + i)) % 5) / 4 for i in range(6)]
    x = torch.stack(cols + [pos[:, 2]], 1)
    x[:, :6] += 0.3 * torch.randn(x.shape[0], 6, generator=gen, device=pos.device)
    return x.float().contiguous()


def rounds(x, S, E, W, min_size, route):
    """Level 0 once more, one round at a time: [(components, edges, device ms)]."""
    B = P._route(x, route)
    F = (x.double() * S.double()[:, None]).contiguous()
    E, W = P.component_graph(None, E, W, "add", num_components=x.shape[0], route=route)
    out = []
    while E.shape[1]:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        best = B.choose(F, S, E, W, REG)
        parent, n_active = B.resolve(best, S, min_size, False)
        if n_active:
            label, num_new = B.relabel(parent)
            S2, F2, _ = B.accumulate(label, num_new, S, F, None)
            E2, W2 = B.component_graph(label, E, W, "add", label.numel(), num_new)
        b.record()
        torch.cuda.synchronize()
        out.append((S.numel(), E.shape[1], n_active, a.elapsed_time(b)))
        if not n_active:
            break
        S, F, E, W = S2, F2, E2, W2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="T")
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--levels", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    pos = make_voxel_cloud(SCENES[a.scene][0], voxel=0.03, seed=4321, device=dev)
    n = pos.shape[0]
    nn, _ = knn_1(pos, K, r_max=2.0)
    src = torch.arange(n, device=dev).repeat_interleave(K)
    dst = nn.reshape(-1)
    keep = dst >= 0
    edge_index = torch.stack([src[keep], dst[keep]]).contiguous()
    del nn, src, dst, keep
    x = features(pos, gen)
    print(f"scene {a.scene}: {n} points, {edge_index.shape[1]} directed kNN edges (k = {K}), D = {D}, "
          f"reg = {REG}, min_size = {MIN_SIZE[:a.levels]}")
    legs = {"new": ("merge kernels", "kernels"), "torch": ("torch composition", "torch")}
    labels = {}
    for key, (name, route) in legs.items():
        if a.leg not in ("all", key):
            continue
        data = Data(x=x, pos=pos, edge_index=edge_index,
                    edge_attr=torch.ones(edge_index.shape[1], device=dev))
        for level, min_size in enumerate(MIN_SIZE[:a.levels]):
            state = {}

            def run():
                state["out"] = P.merge_components_by_contour_prior_on_data(
                    data, REG, min_size, route=route)
            med, wall, peak = timed(run, a.reps)
            d1, (X, S, E, W, Pm, sub) = state["out"]
            labels.setdefault(level, []).append(d1.super_index)
            print(f"{name}, level {level} (min_size {min_size}): {data.num_nodes} -> {S.numel()} components, "
                  f"{data.edge_index.shape[1]} -> {E.shape[1]} edges; device {med:.2f} ms median, host wall "
                  f"{wall:.2f} ms over {a.reps} calls (+ 1 warm-up), peak {peak / 2**20:.0f} MiB")
            if level == 0:
                ones = torch.ones(n, dtype=torch.int64, device=dev)
                for r, (c, e, act, ms) in enumerate(rounds(x, ones, edge_index, None, min_size, route)):
                    print(f"    round {r}: {c} components, {e} edges, {act} active: {ms:.2f} ms")
            data = Data(x=X, pos=Pm, edge_index=E, edge_attr=torch.ones_like(W), node_size=S)
    for level, both in labels.items():
        if len(both) == 2:
            print(f"level {level}: labels of the two legs equal: {torch.equal(both[0], both[1])}")


if __name__ == "__main__":
    main()
