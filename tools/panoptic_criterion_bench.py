"""The panoptic criterion at scene size: ``panoptic.major_objects`` (csrc/panoptic.hip) and
``ops.edge_affinity_loss`` forward + backward (csrc/loss.hip) against the reference's composition
restated in torch on the same device and the same inputs.  The yardstick is that composition,
never the new code itself.

  (a) major objects: the restatement is ``InstanceData.major`` as the package has had it - the
      arg-max segment reduce, the segment sum, and the two ``bool(...)`` host reads of its
      data-dependent branch;
  (b) the loss, forward + backward, with the metric counters: the restatement is
      ``sanitized_edge_affinities()`` (``torch.where`` on the void-edge mask, a host read and a
      data-dependent shape; the two gathers of ``y`` and ``obj``), ``_edge_affinity_weights`` (four
      masked assignments), ``binary_cross_entropy_with_logits(reduction='none', pos_weight)``, the
      weighted mean of ``WeightedLossMixIn`` with its two asserting host reads, ``backward()``,
      and tp / fp / tn / fn as four masked sums;
  (c) both together.

The scene: the level-1 node count of ``synthetic.SCENES``, two edges per node (S: 428 571 nodes,
857 142 edges), objects = as many as the level-2 segments, two overlaps per node, a fifth of the
objects void, a fifth of the nodes more than half void.

    python tools/panoptic_criterion_bench.py [S|T|R] [--reps N] [--rehearse]

``--rehearse``: the new legs once on CPU tensors, nothing timed (no GPU needed; the restatement
of (a) runs on the device only).  Per leg: device-time median and minimum over ``--reps`` calls
after two warm-up calls and a settle pause, host wall median, kernel launches and host reads of
one call.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_bench import host_reads, launches, timed  # noqa: E402
from superpoint_transformer_amd import ops, panoptic, predict  # noqa: E402
from superpoint_transformer_amd.instance import InstanceData  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES  # noqa: E402

C = 13
CASE_WEIGHTS = [0.5, 4.0, 1.0, 2.0]
POS_WEIGHT = 2.5


def scene(name, dev):
    n1, n_obj = SCENES[name][1], SCENES[name][2]
    e = 2 * n1
    gen = torch.Generator(device=dev).manual_seed(20)
    own = (torch.arange(n1, device=dev) * n_obj) // n1
    other = (own + 1 + torch.randint(0, 3, (n1,), generator=gen, device=dev)) % n_obj
    obj = torch.stack((own, other), dim=1).reshape(-1)
    count = torch.randint(1, 400, (2 * n1,), generator=gen, device=dev)
    obj_y = torch.randint(0, C, (n_obj,), generator=gen, device=dev)
    obj_y[torch.rand(n_obj, generator=gen, device=dev) < 0.2] = C
    data = InstanceData(torch.arange(n1 + 1, device=dev) * 2, obj * 3 + 1, count, obj_y[obj])
    hist = torch.randint(0, 30, (n1, C + 1), generator=gen, device=dev)
    hist[:, C] = torch.where(torch.rand(n1, generator=gen, device=dev) < 0.2, 1000, 0)
    src = torch.randint(0, n1, (e,), generator=gen, device=dev)
    dst = (src + 1 + torch.randint(0, 40, (e,), generator=gen, device=dev)) % n1
    ei = torch.stack((torch.minimum(src, dst), torch.maximum(src, dst))).contiguous()
    target = torch.rand(e, generator=gen, device=dev)
    logits = torch.randn(e, generator=gen, device=dev) * 3
    return data, hist, ei, target, logits


def torch_loss(logits, target, ei, void, obj, y, cw, pw):
    """``model_step``'s edge-affinity part and the step's metric counters, as the reference
    composes them; returns (loss, d loss / d logits, counters)."""
    x = logits.detach().requires_grad_()
    mask = void[ei]
    idx = torch.where(~(mask[0] & mask[1]))[0]                         # sanitized_edge_affinities
    same_class = (y[ei[0]] == y[ei[1]])[idx]
    same_obj = (obj[ei[0]] == obj[ei[1]])[idx]
    pred, tgt = x[idx], target[idx]
    w = torch.ones_like(same_class).float()                            # _edge_affinity_weights
    w[same_class * same_obj] = cw[0]
    w[same_class * ~same_obj] = cw[1]
    w[~same_class * same_obj] = cw[2]
    w[~same_class * ~same_obj] = cw[3]
    assert w.ge(0).all() and w.gt(0).any()                             # WeightedLossMixIn
    l = torch.nn.functional.binary_cross_entropy_with_logits(pred, tgt, pos_weight=pw,
                                                             reduction="none")
    loss = (l.view(-1, 1) * (w / w.sum()).view(-1, 1)).sum()
    loss.backward()
    p, t = pred.detach() > 0, tgt > 0.5
    stats = torch.stack(((p & t).sum(), (p & ~t).sum(), (~p & ~t).sum(), (~p & t).sum()))
    return loss.detach(), x.grad, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cpu" if a.rehearse else "cuda:0")
    data, hist, ei, target, logits = scene(a.scene, dev)
    void = predict.void_mask(hist)
    cw = torch.tensor(CASE_WEIGHTS, device=dev)
    pw = torch.tensor([POS_WEIGHT], device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)

    def new_major():
        return panoptic.major_objects(data, C, check=False)

    def new_loss(obj, y):
        x = logits.detach().requires_grad_()
        stats.zero_()
        loss = ops.edge_affinity_loss(x, target, ei, void, obj, y, case_weights=cw, pos_weight=pw,
                                      stats=stats)
        loss.backward()
        return loss.detach(), x.grad, stats

    obj, _, y = new_major()
    loss, grad, st = new_loss(obj, y)
    print(f"scene {a.scene}: {data.num_groups} nodes, {data.num_items} pairs, {ei.shape[1]} edges, "
          f"{int(void.sum())} void nodes, C = {C}; loss {float(loss):.7f}, counters {st.tolist()}")
    if a.rehearse:
        return
    ref_major = data.major(C)
    print(f"(a) major objects equal to InstanceData.major: "
          f"{all(torch.equal(p, q) for p, q in zip(new_major(), ref_major))}")
    ref_loss, ref_grad, ref_stats = torch_loss(logits, target, ei, void, obj, y, CASE_WEIGHTS, pw)
    scale = float(ref_grad.abs().max())
    print(f"(b) loss {float(loss):.7f} against the restatement's {float(ref_loss):.7f} (f32 sums "
          f"there); largest gradient difference / largest gradient "
          f"{float((grad - ref_grad).abs().max()) / scale:.2e}; counters equal: "
          f"{torch.equal(st, ref_stats)}")

    def new_both():
        o, _, yy = new_major()
        return new_loss(o, yy)

    def torch_both():
        o, _, yy = data.major(C)
        return torch_loss(logits, target, ei, void, o, yy, CASE_WEIGHTS, pw)

    table = [("a", "new, major_objects()", new_major),
             ("a", "torch, InstanceData.major()", lambda: data.major(C)),
             ("b", "new, edge_affinity_loss fwd + bwd + counters", lambda: new_loss(obj, y)),
             ("b", "torch, sanitize + weights + BCE + bwd + counters",
              lambda: torch_loss(logits, target, ei, void, obj, y, CASE_WEIGHTS, pw)),
             ("c", "new, both", new_both),
             ("c", "torch, both", torch_both)]
    print(f"{'leg':<56}{'ms median':>11}{'ms min':>9}{'wall ms':>9}{'launches':>10}{'host reads':>12}")
    for group, name, fn in table:
        med, best, wall = timed(fn, a.reps)
        print(f"({group}) {name:<52}{med:>11.3f}{best:>9.3f}{wall:>9.2f}{launches(fn):>10}"
              f"{host_reads(fn):>12}")


if __name__ == "__main__":
    main()
