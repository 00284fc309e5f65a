"""The sparse convolution at batch and scene size: the device route (the kernels of
csrc/sparse_conv.hip) against a torch restatement of the gather -> GEMM -> scatter-add dataflow on
device tensors (the package's own composition: map from sort / ``searchsorted``, per offset
gather, matmul, ``index_add``; autograd for the backward).

The voxels are those of a voxelised synthetic cloud (``voxel_groups(...).coords``).  Layers:
``C_in -> 32`` with K = 7 and ``32 -> 32`` with K = 3; legs, each timed on its own: map build,
forward, forward + backward, and the whole ``[C_in, 32, 32, 32]`` CNN (GraphNorm + LeakyReLU)
with kernel sizes ``[7, 3, 3]`` and ``3``.  Reported with them: pairs per voxel, peak memory,
host reads of a map build.

    python tools/sparse_conv_bench.py [T|S] [--leg all|new|torch] [--reps N] [--cin C] [--no-k7-torch]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import sparse as S  # noqa: E402
from superpoint_transformer_amd.nn.sparse import SparseCNN, SparseTensor  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES, make_voxel_cloud  # noqa: E402
from superpoint_transformer_amd.voxel import voxel_groups  # noqa: E402


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


def line(name, what, res):
    med, wall, peak = res
    print(f"  {name:18s} {what:22s} device {med:9.2f} ms median, host wall {wall:9.2f} ms, "
          f"peak {peak / 2**20:8.0f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="T")
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cin", type=int, default=7)
    ap.add_argument("--no-k7-torch", action="store_true",
                    help="skip the torch restatement of the K = 7 legs (343 searches, 8-byte pairs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pos = make_voxel_cloud(SCENES[a.scene][0], voxel=0.03, seed=4321, device=dev)
    coords = voxel_groups(pos, 0.03).coords.contiguous()
    del pos
    n = coords.shape[0]
    gen = torch.Generator(device=dev).manual_seed(5)
    print(f"scene {a.scene}: {n} voxels; C_in = {a.cin}; {a.reps} timed calls after one warm-up each",
          flush=True)
    legs = {"new": "sparse_conv kernels", "torch": "torch restatement"}
    for K, ci in ((7, a.cin), (3, 32)):
        x = torch.randn(n, ci, generator=gen, device=dev)
        W = torch.randn(K ** 3, ci, 32, generator=gen, device=dev) * 0.05
        g = torch.randn(n, 32, generator=gen, device=dev)
        outs = {}
        for key, name in legs.items():
            if a.leg not in ("all", key) or (key == "torch" and K == 7 and a.no_k7_torch):
                continue
            print(f"layer {ci} -> 32, K = {K}: {name}", flush=True)
            build = (lambda: S.build_kernel_map(coords, None, K, 1)) if key == "new" else \
                (lambda: S._map_torch(coords, None, n, K, 1))
            state = {}

            def run_build():
                state["map"] = None
                state["map"] = build()
            line(name, "map build", timed(run_build, a.reps))
            kmap = state["map"]
            reads = "2 (bounds record; pairs, duplicates)" if key == "new" else \
                "3 + K^3 (bounds, duplicates, pair count; the searches sync per offset)"
            print(f"    {kmap.num_pairs} pairs, {kmap.pairs_per_voxel:.2f} per voxel; host reads of a "
                  f"build: {reads}", flush=True)
            xs, Ws = x.clone().requires_grad_(), W.clone().requires_grad_()

            def fwd():
                with S.composition_only(key == "torch"), torch.no_grad():
                    state["out"] = S.sparse_conv3d(xs, Ws, kmap)

            def fwd_bwd():
                with S.composition_only(key == "torch"):
                    out = S.sparse_conv3d(xs, Ws, kmap)
                    state["grads"] = torch.autograd.grad(out, (xs, Ws), g)
            line(name, "forward", timed(fwd, a.reps))
            line(name, "forward + backward", timed(fwd_bwd, a.reps))
            outs[key] = (state["out"], *state["grads"])
            state.clear()
            del kmap
        if len(outs) == 2:
            for what, u, v in zip(("out", "dX", "dW"), outs["new"], outs["torch"]):
                print(f"    {what}: max |kernels - torch| {(u - v).abs().max().item():.3e} of "
                      f"{v.abs().max().item():.3e}", flush=True)
        del outs, x, W, g
    for ks in ([7, 3, 3], 3):
        torch.manual_seed(0)
        cnn = SparseCNN([a.cin, 32, 32, 32], ks, 1, activation=torch.nn.LeakyReLU()).to(dev)
        x = torch.randn(n, a.cin, generator=gen, device=dev)
        c4 = torch.cat([coords.new_zeros(n, 1), coords], 1)
        for key, name in legs.items():
            if a.leg not in ("all", key) or (key == "torch" and ks != 3 and a.no_k7_torch):
                continue

            def net():
                with S.composition_only(key == "torch"):
                    real = S.build_kernel_map
                    if key == "torch":
                        S.build_kernel_map = lambda c, b, k, d: S._map_torch(c.contiguous(), b, n, k, d)
                    try:
                        out = cnn(SparseTensor(coords=c4, feats=x)).F
                        out.square().mean().backward()
                    finally:
                        S.build_kernel_map = real
            line(name, f"CNN {ks} fwd+bwd+maps", timed(net, a.reps))


if __name__ == "__main__":
    main()
