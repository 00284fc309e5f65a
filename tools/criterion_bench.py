"""The default semantic criterion ('ce_kl' with class weights, forward + backward) at the level
sizes of a scene: the histogram-loss kernels (criterion.SemanticCriterion) against a torch
restatement of the reference's composition (mask -> repeat_interleave -> where -> weighted
reduction='none' CE: two data-dependent sizes = two host round trips per level), and the parent's
unweighted ops.cross_entropy at the level-1 size as the yardstick of the kernel itself.

    python tools/criterion_bench.py [S|T] [--leg all|new|torch|ce] [--reps N]

``--leg`` other than ``all`` runs that leg alone, for a kernel trace of its own:
    rocprofv3 --kernel-trace -d <dir> -- python tools/criterion_bench.py S --leg new
    python tools/rocpd_summary.py <dir>
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import ops  # noqa: E402
from superpoint_transformer_amd.criterion import SemanticCriterion  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES  # noqa: E402

C, LAMBDAS = 13, (1.0, 50.0)


def make_level(rows, gen, dev):
    """Logits and a sparse label histogram (about 2.5 classes per superpoint, void included)."""
    z = torch.randn(rows, C, device=dev, generator=gen) * 3
    h = (torch.randint(1, 200, (rows, C + 1), device=dev, generator=gen)
         * (torch.rand(rows, C + 1, device=dev, generator=gen) < 0.18))
    return z.requires_grad_(), h


def composition_hist(z, h, w):
    """What the reference's loss_with_target_histogram does, restated: one CE term per non-zero
    histogram cell on a row-expanded copy of the logits, weighted by the cell's share."""
    mask = h != 0
    zf = z.repeat_interleave(mask.sum(dim=1), dim=0)            # host round trip (output size)
    cls = torch.where(mask)[1]                                  # host round trip (output size)
    share = h[mask]
    share = share.float() / share.sum()
    per = torch.nn.functional.cross_entropy(zf, cls, weight=w, ignore_index=C, reduction="none")
    return (per * share).sum()


def composition_ce_kl(zs, hs, w):
    loss = torch.nn.functional.cross_entropy(zs[0], hs[0].argmax(dim=1), weight=w, ignore_index=C)
    return loss + LAMBDAS[1] * composition_hist(zs[1], hs[1], w)


def timed(fn, reps, settle=0.3):
    for _ in range(3):
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
    ap.add_argument("--leg", default="all", choices=["all", "new", "torch", "ce"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n1, n2 = SCENES[a.scene][1:3]
    gen = torch.Generator(device=dev).manual_seed(7)
    (z1, h1), (z2, h2) = make_level(n1, gen, dev), make_level(n2, gen, dev)
    w = 0.4 + 1.6 * torch.rand(C, device=dev, generator=gen)
    labels = torch.randint(0, C, (n1,), device=dev, generator=gen)
    crit = SemanticCriterion(C, "ce_kl", LAMBDAS, weight=w).to(dev)

    def new():
        torch.autograd.grad(crit([z1, z2], [h1, h2]), [z1, z2])

    def composition():
        torch.autograd.grad(composition_ce_kl([z1, z2], [h1, h2], w), [z1, z2])

    def plain_ce():
        torch.autograd.grad(ops.cross_entropy(z1, labels), [z1])

    if a.leg == "all":                                          # (a traced leg runs nothing but itself)
        ref, mine = composition_ce_kl([z1, z2], [h1, h2], w), crit([z1, z2], [h1, h2])
        print(f"scene {a.scene}: levels of {n1} and {n2} rows, C = {C}, {int((h1 != 0).sum())} + "
              f"{int((h2 != 0).sum())} non-zero histogram cells; loss kernels {float(mine):.7g}, "
              f"torch composition {float(ref):.7g}")
    legs = {"new": ("ce_kl + weights, fwd + bwd, histogram-loss kernels (2 levels)", new),
            "torch": ("ce_kl + weights, fwd + bwd, torch composition (2 levels)", composition),
            "ce": (f"unweighted ops.cross_entropy fwd + bwd, {n1} rows", plain_ce)}
    for key, (name, fn) in legs.items():
        if a.leg in ("all", key):
            med, best, wall = timed(fn, a.reps)
            print(f"{name}: device {med:.3f} ms median / {best:.3f} ms min, "
                  f"host wall {wall:.3f} ms median over {a.reps} calls (+ 3 warm-up calls)")


if __name__ == "__main__":
    main()
