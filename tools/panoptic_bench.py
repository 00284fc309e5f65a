"""Panoptic evaluation at scene size: ``output.PanopticSegmentationOutput.panoptic_pred`` and
``metrics.PanopticQuality3D.update`` (the kernels of csrc/panoptic.hip) against the reference's
composition restated in torch on the same device and the same inputs.  The yardstick is that
composition, never the new code itself.

  (a) ``panoptic_pred()``: the restatement is ``InstanceData.merge`` as the package has had it
      (``torch.unique`` / ``argsort`` / ``repeat_interleave`` passes and their host reads) and
      ``scatter_mean_weighted`` as ``index_add_`` of ``cat(w, x * w)``, then softmax / max;
  (b) ``update()``: the restatement moves ``obj_y`` and the merged ``InstanceData`` to the CPU,
      as the reference's ``validation_step`` does per batch, and counts what its ``compute()``
      counts for this batch on the device: ``remove_void``, ``iou_and_size``, the relabelling of
      the objects, the bincounts and the two scatter sums;
  (c) both together.

The scene: the level-1 node count of ``synthetic.SCENES``, objects = as many as its level-2
segments with sparse ids 3k + 1, two overlaps per node (its own object and a neighbour), a fifth
of the objects void, predicted instances = the nodes' own object with one node in ten moved to
a neighbour.

    python tools/panoptic_bench.py [S|T|R] [--reps N] [--rehearse]

``--rehearse``: the new legs once on CPU tensors, nothing timed (no GPU needed; the restatement
runs on the device only).  Per leg: device-time median and minimum over ``--reps`` calls after two
warm-up calls and a settle pause, host wall median, kernel launches and host reads of one call.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_bench import host_reads, launches, timed  # noqa: E402
from superpoint_transformer_amd.instance import InstanceData, _consecutive  # noqa: E402
from superpoint_transformer_amd.metrics import PanopticQuality3D  # noqa: E402
from superpoint_transformer_amd.output import PanopticSegmentationOutput  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES  # noqa: E402

C, STUFF = 13, [0, 1, 2]


def scene(name, dev):
    n1, n_obj = SCENES[name][1], SCENES[name][2]
    gen = torch.Generator(device=dev).manual_seed(19)
    own = (torch.arange(n1, device=dev) * n_obj) // n1
    other = (own + 1 + torch.randint(0, 3, (n1,), generator=gen, device=dev)) % n_obj
    obj = torch.stack((torch.minimum(own, other), torch.maximum(own, other)), dim=1).reshape(-1)
    count = torch.randint(1, 400, (2 * n1,), generator=gen, device=dev)
    obj_y = torch.randint(0, C, (n_obj,), generator=gen, device=dev)
    obj_y[torch.rand(n_obj, generator=gen, device=dev) < 0.2] = C
    data = InstanceData(torch.arange(n1 + 1, device=dev) * 2, obj * 3 + 1, count, obj_y[obj])
    moved = torch.rand(n1, generator=gen, device=dev) < 0.1
    idx = torch.where(moved, other, own)
    idx = torch.unique(idx, return_inverse=True)[1].contiguous()       # dense in [0, max]
    logits = torch.randn(n1, C, generator=gen, device=dev)
    node_size = torch.randint(1, 300, (n1,), generator=gen, device=dev)
    return data, idx, logits, node_size


def output(data, idx, logits, node_size):
    dev, n1 = logits.device, logits.shape[0]
    z = torch.zeros(1, device=dev)
    return PanopticSegmentationOutput(
        logits, STUFF, z, node_size, y_hist=torch.zeros(n1, C + 1, dtype=torch.long, device=dev),
        obj=data, obj_edge_index=torch.zeros(2, 1, dtype=torch.long, device=dev),
        obj_edge_affinity=z, pos=torch.zeros(n1, 3, device=dev),
        obj_pos=torch.zeros(n1, 3, device=dev), obj_index_pred=idx)


def torch_pred(data, idx, logits, node_size):
    merged = data.merge(idx)
    w = node_size.view(-1, 1).float()
    wx = torch.cat((w, logits * w), dim=1)
    seg = torch.zeros(int(idx.max()) + 1, C + 1, device=logits.device).index_add_(0, idx, wx)
    w_seg = seg[:, 0]
    w_seg[w_seg == 0] = 1
    score, y = (seg[:, 1:] / w_seg.view(-1, 1)).softmax(dim=1).max(dim=1)
    return score, y, merged


def torch_update(pred, merged, is_stuff):
    """One batch of the reference's ``update`` (the moves to the CPU) and of its ``compute``
    (src/metrics/panoptic.py:225-323) on the device; returns the five counters."""
    pred.cpu(), [t.cpu() for t in (merged.pointers, merged.obj, merged.count, merged.y)]
    pair_data, valid = merged.remove_void(C)
    pred = pred[valid]
    pair_pred_idx = pair_data.indices
    pair_iou = pair_data.iou_and_size()[0]
    pair_gt_idx, gt_idx = _consecutive(pair_data.obj)
    gt_semantic = pair_data.y[gt_idx]
    gt_counts = torch.bincount(gt_semantic, minlength=C)
    pred_counts = torch.bincount(pred, minlength=C)
    pair_gt = gt_semantic[pair_gt_idx]
    agrees = pair_gt == pred[pair_pred_idx]
    gt50 = pair_iou > 0.5
    sel = torch.where(agrees & gt50)[0]
    tp = torch.bincount(pair_gt[sel], minlength=C)
    iou_sum = torch.zeros(C, device=pred.device).index_add_(0, pair_gt[sel], pair_iou[sel])
    sel = torch.where(agrees & (gt50 | is_stuff[pair_gt]))[0]
    iou_mod = torch.zeros(C, device=pred.device).index_add_(0, pair_gt[sel], pair_iou[sel])
    return tp, gt_counts, pred_counts, iou_sum, iou_mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cpu" if a.rehearse else "cuda:0")
    data, idx, logits, node_size = scene(a.scene, dev)
    out = output(data, idx, logits, node_size)
    pq = PanopticQuality3D(C, stuff_classes=STUFF, device=dev)
    is_stuff = torch.tensor([c in STUFF for c in range(C)], device=dev)
    score, obj_y, merged = out.panoptic_pred()
    print(f"scene {a.scene}: {data.num_groups} nodes, {data.num_items} pairs, "
          f"{int(torch.unique(data.obj).numel())} objects -> {merged.num_groups} predicted "
          f"instances, {merged.num_items} merged pairs, C = {C}")
    pq.update(obj_y, merged)
    if a.rehearse:
        print("PQ of the new route:", float(pq.compute().pq))
        return
    ref_score, ref_y, ref_merged = torch_pred(data, idx, logits, node_size)
    same = all(torch.equal(getattr(merged, k), getattr(ref_merged, k))
               for k in ("pointers", "obj", "count", "y"))
    print(f"(a) merged InstanceData equal to the restatement's: {same}; labels equal: "
          f"{float((obj_y == ref_y).float().mean()):.6f} of the instances; largest score "
          f"difference {float((score - ref_score).abs().max()):.2e}")
    ref = torch_update(ref_y, ref_merged, is_stuff)
    pq.reset()
    pq.update(ref_y, merged)
    print(f"(b) tp / gt_count / pred_count equal to the restatement's: "
          f"{all(torch.equal(x, y) for x, y in zip((pq.tp, pq.gt_count, pq.pred_count), ref[:3]))}; "
          f"largest relative difference of the IoU sums (f64 fixed point against f32 "
          f"index_add_): {float(((pq.iou_sum - ref[3]).abs() / ref[3].clamp(min=1)).max()):.2e}")

    def new_update():
        pq.update(obj_y, merged)

    def new_both():
        s, y, m = out.panoptic_pred()
        pq.update(y, m)

    def torch_both():
        s, y, m = torch_pred(data, idx, logits, node_size)
        torch_update(y, m, is_stuff)

    from superpoint_transformer_amd import panoptic
    table = [("a", "new, merge_instances() alone", lambda: panoptic.merge_instances(data, idx)),
             ("a", "new, panoptic_pred()", out.panoptic_pred),
             ("a", "torch, merge + scatter_mean_weighted", lambda: torch_pred(data, idx, logits, node_size)),
             ("b", "new, update()", new_update),
             ("b", "torch, .cpu() + the batch's share of compute()",
              lambda: torch_update(ref_y, ref_merged, is_stuff)),
             ("c", "new, panoptic_pred() + update()", new_both),
             ("c", "torch, both", torch_both),
             ("-", "new, compute()", pq.compute)]
    print(f"{'leg':<56}{'ms median':>11}{'ms min':>9}{'wall ms':>9}{'launches':>10}{'host reads':>12}")
    for group, name, fn in table:
        med, best, wall = timed(fn, a.reps)
        print(f"({group}) {name:<52}{med:>11.3f}{best:>9.3f}{wall:>9.2f}{launches(fn):>10}"
              f"{host_reads(fn):>12}")


if __name__ == "__main__":
    main()
