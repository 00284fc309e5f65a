"""Superedges at scene size: ``graph.superedge_features`` (csrc/superedge.hip) against the route
the package had before it - ``graph.subedges`` plus the torch evaluation of the 7 features,
chunked at the reference's 100 000 edges - on the same device and the same inputs, and the whole
``transforms.RadiusHorizontalGraph`` with its share per step.  The yardstick is that composition,
never the new code itself.

The scene: ``synthetic.make_nag`` (S, T or R), the level-1 and level-2 edge lists it carries
(trimmed), level-0 points as the segments' members.  Per level and route: device-time median and
minimum over ``--reps`` calls after warm-up calls and a settle pause, host wall median, peak
device memory above what the inputs hold, kernel launches and host reads of one call; the largest
difference of ``mean_off`` between the two routes as a sanity figure.

    python tools/superedge_bench.py [S|T|R] [--reps N] [--rehearse]

``--rehearse``: scene R once through both routes on CPU tensors, nothing timed (no GPU needed).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_bench import host_reads, launches, timed  # noqa: E402
from superpoint_transformer_amd import graph as G  # noqa: E402
from superpoint_transformer_amd.synthetic import make_nag  # noqa: E402

CHUNK = 100_000
KW = dict(ratio=0.2, k_min=20, cycles=3, margin=0.2)


def composition(pos, index, ei, num_segments):
    """The route before the kernel: chunks of 100 000 trimmed edges through ``subedges`` and the
    torch features (src/transforms/graph.py:742-796 with its ``chunk_size``)."""
    out = []
    for c in range(0, ei.shape[1], CHUNK):
        sub = ei[:, c:c + CHUNK]
        _, pairs, uid = G.subedges(pos, index, sub, **KW)
        out.append(G.minimalistic_edge_features(pos, pairs, uid, sub.shape[1]))
    return torch.cat(out) if out else pos.new_empty((0, 7))


def peak_of(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def levels_of(nag):
    si0, si1 = nag[0]["super_index"], nag[1]["super_index"]
    return {1: (si0, nag[1]["pos"].shape[0], G.to_trimmed(nag[1]["edge_index"])),
            2: (si1[si0], nag[2]["pos"].shape[0], G.to_trimmed(nag[2]["edge_index"]))}


def rehearse():
    nag = make_nag("R", seed=7, device="cpu")
    pos = nag[0]["pos"]
    for lv, (index, n, ei) in levels_of(nag).items():
        ei = ei[:, :400]
        _, attr = G.superedge_features(pos, index, ei, num_segments=n, **KW)
        ref = composition(pos, index, ei, n)
        print(f"level {lv}: {ei.shape[1]} edges, |mean_off difference| max "
              f"{float((attr - ref)[:, :3].abs().max()):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--skip-composition", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        return rehearse()
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.data import Data, NAG
    from superpoint_transformer_amd.neighbors import cluster_radius_nn_graph
    dev = torch.device("cuda:0")
    print(f"box: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, scene {args.scene}, "
          f"reps {args.reps}, capacity C = {G.superedge_capacity()}", flush=True)
    nag = make_nag(args.scene, seed=1234, device=dev)
    pos = nag[0]["pos"].contiguous()
    C = G.superedge_capacity()
    for lv, (index, n, ei) in levels_of(nag).items():
        index = index.contiguous()
        size = torch.bincount(index, minlength=n)
        big = size[ei].max(0).values
        print(f"\nlevel {lv}: {n} segments of {int(size.min())} .. {int(size.max())} points (mean "
              f"{float(size.float().mean()):.1f}), {ei.shape[1]} trimmed edges: {int((big <= 64).sum())} "
              f"small, {int(((big > 64) & (big <= C)).sum())} medium, {int((big > C).sum())} large",
              flush=True)
        legs = [("kernel", lambda: G.superedge_features(pos, index, ei, num_segments=n, **KW)[1])]
        if not args.skip_composition:
            legs.append(("composition", lambda: composition(pos, index, ei, n)))
        res = {}
        for name, fn in legs:
            med, best, wall = timed(fn, args.reps)
            res[name], peak = peak_of(fn, dev)
            small = name == "kernel" or ei.shape[1] <= 1_000_000     # the long leg is not run twice more
            print(f"  {name:<12} device {med:9.2f} ms (min {best:9.2f})  wall {wall:9.2f} ms  peak "
                  f"{peak:9.1f} MiB  launches {launches(fn) if small else '-'}  host reads "
                  f"{host_reads(fn) if small else '-'}", flush=True)
        if len(res) == 2:
            d = (res["kernel"] - res["composition"]).abs()
            # mean_off does not depend on the pairing: an edge where it differs selected another
            # point (a key within rounding of a threshold; the composition projects by a library
            # product), an edge where only the other columns differ was paired in the other direction
            off = d[:, :3].max(dim=1).values
            print(f"  |kernel - composition| max: mean_off {float(off.max()):.3e}, all columns "
                  f"median {float(d.median()):.3e}; edges with another point set (mean_off apart by "
                  f"more than 1e-4): {int((off > 1e-4).sum())} of {d.shape[0]}; paired in the other "
                  f"direction: {int(((off <= 1e-4) & (d[:, 3:].max(dim=1).values > 1e-4)).sum())}")

    # the whole transform, step by step (k_max 30, gap 0.2: every level gets edges and isolated nodes)
    data = NAG([Data(pos=nag[0]["pos"], super_index=nag[0]["super_index"]),
                Data(pos=nag[1]["pos"], super_index=nag[1]["super_index"], batch=nag[1]["batch"]),
                Data(pos=nag[2]["pos"], batch=nag[2]["batch"])])
    tr = T.RadiusHorizontalGraph(k_min=1, k_max=30, gap=0.2)
    med, best, wall = timed(lambda: tr(data), max(args.reps // 2, 2))
    print(f"\nRadiusHorizontalGraph(k_max=30, gap=0.2): device {med:.2f} ms (min {best:.2f}), wall "
          f"{wall:.2f} ms, host reads {host_reads(lambda: tr(data))}")

    def step(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    for lv in (1, 2):
        d, si = data[lv], data.get_super_index(lv)
        e0, t_r = step(lambda: cluster_radius_nn_graph(pos, si, k_max=30, gap=0.2, batch=d.batch,
                                                       num_clusters=d.num_nodes)[0])
        e1, t_c = step(lambda: G.connect_isolated(e0, d.pos, 1, batch=d.batch, num_nodes=d.num_nodes))
        e2, t_t = step(lambda: G.to_trimmed(e1))
        _, t_s = step(lambda: G.superedge_features(pos, si, e2, num_segments=d.num_nodes, **KW))
        tot = t_r + t_c + t_t + t_s
        print(f"  level {lv}: {e0.shape[1]} radius edges + {e1.shape[1] - e0.shape[1]} for isolated nodes "
              f"-> {e2.shape[1]} trimmed; wall ms: radius graph {t_r:.1f} ({100 * t_r / tot:.0f} %), "
              f"connect_isolated {t_c:.1f} ({100 * t_c / tot:.0f} %), to_trimmed {t_t:.1f} "
              f"({100 * t_t / tot:.0f} %), superedge_features {t_s:.1f} ({100 * t_s / tot:.0f} %)")


if __name__ == "__main__":
    main()
