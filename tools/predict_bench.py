"""Predictions back to the cloud at scene size: ``output.SemanticSegmentationOutput`` /
``output.MultiRunInference`` (the kernels of csrc/predict.hip) against the reference's composition
restated in torch on the same device and the same inputs.  The yardstick is that composition,
never the new code itself.

  (a) full-resolution prediction: ``argmax``, ``[si01][si_raw0]``; starting from the stored
      Clusters the composition first runs ``to_super_index()`` on both (``arange`` /
      ``repeat_interleave`` / scatter);
  (b) full-resolution confusion matrix: the composition materialises the prediction, then one
      ``index_add_`` of ones at ``target * C + pred`` over the non-void points; the new route
      writes no prediction;
  (c) three-run accumulation plus propagation: ``logits[node_id] += run_logits`` and
      ``seen[node_id] = True`` per run, then the nearest seen neighbour of every unseen node (the
      package's ``knn_2`` on both sides) and the copy.

The hierarchy: the scene's superpoint and voxel counts, ``--per-voxel`` raw points per voxel
(default 4), skewed cluster sizes (a few superpoints of thousands of voxels among small ones),
raw points in shuffled order, Clusters with the points of a cluster ascending (as
``GridSampling3D`` and the partition store them).

    python tools/predict_bench.py [S|T|R] [--reps N] [--per-voxel K] [--rehearse]

``--rehearse``: every leg once on CPU tensors, results compared, nothing timed (no GPU needed).
Per leg: device-time median and minimum over ``--reps`` calls after two warm-up calls and a
settle pause, host wall median, kernel launches and host reads of one call.
"""
import argparse
import logging
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd.data import NAG, Cluster, Data  # noqa: E402
from superpoint_transformer_amd.output import MultiRunInference, SemanticSegmentationOutput  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES  # noqa: E402

C, KEY = 13, "tta_node_id"


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


def launches(fn):
    """Kernels of one run, counted by the profiler (-1 where it is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return sum(1 for n in names if "memcpy" not in n.lower() and "memset" not in n.lower())
    except Exception:
        return -1


def sorted_cluster(si, n_clusters):
    """The Cluster of a super_index, the points of every cluster ascending."""
    order = torch.sort(si, stable=True).indices
    sizes = torch.bincount(si, minlength=n_clusters)
    return Cluster(torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]), order, ascending=True)


def hierarchy(scene, per_voxel, dev):
    n_vox, n_sp = SCENES[scene][0], SCENES[scene][1]
    n_raw = per_voxel * n_vox
    gen = torch.Generator(device=dev).manual_seed(77)
    # skew: the cube of a uniform draw puts thousands of voxels into the first superpoints
    si01 = (torch.rand(n_vox, generator=gen, device=dev) ** 3 * n_sp).long().clamp_(max=n_sp - 1)
    si_raw0 = torch.arange(n_vox, device=dev).repeat_interleave(per_voxel)
    si_raw0 = si_raw0[torch.randperm(n_raw, generator=gen, device=dev)].contiguous()
    f = dict(si01=si01, si_raw0=si_raw0, sub1=sorted_cluster(si01, n_sp),
             sub0=sorted_cluster(si_raw0, n_vox),
             logits=torch.randn(n_sp, C, generator=gen, device=dev),
             y_raw=torch.randint(0, C + 1, (n_raw,), generator=gen, device=dev),
             pos=torch.rand(n_sp, 3, generator=gen, device=dev) * torch.tensor(
                 [200.0, 200.0, 10.0], device=dev))
    runs = []
    for r in range(3):
        keep = torch.rand(n_sp, generator=gen, device=dev) < 0.6
        ids = torch.where(keep)[0]
        ids = ids[torch.randperm(ids.numel(), generator=gen, device=dev)].contiguous()
        runs.append((ids, torch.randn(ids.numel(), C, generator=gen, device=dev)))
    f["runs"] = runs
    return f


def to_super_index(cl):
    """Cluster.to_super_index() of the reference (src/data/cluster.py:67-77)."""
    out = torch.empty(cl.num_points, dtype=torch.int64, device=cl.device)
    out[cl.points] = torch.arange(cl.num_clusters, device=cl.device).repeat_interleave(cl.sizes)
    return out


def composition_matrix(pred, y):
    cm = torch.zeros(C * C, dtype=torch.int64, device=y.device)
    ok = (y >= 0) & (y < C)
    cm.index_add_(0, y[ok] * C + pred[ok], torch.ones_like(y[ok]))
    return cm.view(C, C)


def legs(f, mri, nag):
    out = SemanticSegmentationOutput(f["logits"])
    ii = dict(super_index_level0_to_level1=f["si01"], super_index_raw_to_level0=f["si_raw0"])
    cc = dict(sub_level1_to_level0=f["sub1"], sub_level0_to_raw=f["sub0"])
    ic = dict(super_index_level0_to_level1=f["si01"], sub_level0_to_raw=f["sub0"])

    def torch_pred_ii():
        return torch.argmax(f["logits"], dim=1)[f["si01"]][f["si_raw0"]]

    def torch_pred_cc():
        return torch.argmax(f["logits"], dim=1)[to_super_index(f["sub1"])][to_super_index(f["sub0"])]

    def new_multi():
        om = mri.empty_output(nag)
        for ids, z in f["runs"]:
            mri.update(om, SemanticSegmentationOutput(z), [None, {KEY: ids}])
        return mri.finalize(om, nag).logits

    def torch_multi():
        n_sp = f["logits"].shape[0]
        logits = torch.zeros(n_sp, C, device=f["logits"].device)
        seen = torch.zeros(n_sp, dtype=torch.bool, device=logits.device)
        for ids, z in f["runs"]:
            logits[ids] += z
            seen[ids] = True
        unseen_idx = torch.where(~seen)[0]
        if unseen_idx.shape[0] > 0:
            seen_idx = torch.where(seen)[0]
            neighbors = mri._nearest_seen(f["pos"], None, seen_idx, unseen_idx)
            (neighbors == -1).sum().item()                      # the reference's num_left_out read
            logits[unseen_idx] = logits[seen_idx][neighbors]
        return logits

    return [
        ("a", "new, index + index", lambda: out.full_res_semantic_pred(**ii)),
        ("a", "new, index + index, check=False", lambda: out.full_res_semantic_pred(check=False, **ii)),
        ("a", "new, index + Cluster", lambda: out.full_res_semantic_pred(**ic)),
        ("a", "new, Cluster + Cluster", lambda: out.full_res_semantic_pred(**cc)),
        ("a", "torch, argmax[si01][si_raw0]", torch_pred_ii),
        ("a", "torch, to_super_index() x 2 + gathers", torch_pred_cc),
        ("b", "new, index + index, no prediction written",
         lambda: out.confusion_matrix(C, f["y_raw"], "raw", **ii)),
        ("b", "new, Cluster + Cluster, no prediction written",
         lambda: out.confusion_matrix(C, f["y_raw"], "raw", **cc)),
        ("b", "torch, prediction + index_add_", lambda: composition_matrix(torch_pred_ii(), f["y_raw"])),
        ("b", "torch, from Clusters + index_add_", lambda: composition_matrix(torch_pred_cc(), f["y_raw"])),
        ("c", "new, 3 x accumulate_rows_ + finalize", new_multi),
        ("c", "torch, 3 x index_put + seen + propagate", torch_multi),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="S")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--per-voxel", type=int, default=4)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cpu" if a.rehearse else "cuda:0")
    # (the left-out warning of finalize is not part of what is timed)
    logging.getLogger("superpoint_transformer_amd.output").setLevel(logging.ERROR)
    f = hierarchy(a.scene, a.per_voxel, dev)
    n_sp, n_vox, n_raw = f["logits"].shape[0], f["si01"].numel(), f["si_raw0"].numel()
    sizes = f["sub1"].sizes
    print(f"scene {a.scene}: {n_raw} raw points -> {n_vox} voxels -> {n_sp} superpoints, C = {C}; "
          f"largest superpoint {int(sizes.max())} voxels, median {int(sizes.median())}")
    mri = MultiRunInference(C, multi_stage=False, key=KEY, r_max=2)
    nag = NAG([Data(pos=torch.zeros(1, 3, device=dev)), Data(pos=f["pos"])])
    table = legs(f, mri, nag)
    first = {}
    for group, name, fn in table:                         # every leg of a group computes the same
        res = fn()
        if group in first:
            same = bool(torch.equal(res, first[group])) if res.dtype != torch.float32 else \
                bool((res == first[group]).all())
            print(f"({group}) {name}: equal to the group's first leg: {same}")
        else:
            first[group] = res
    del first
    if a.rehearse:
        return
    print(f"{'leg':<52}{'ms median':>11}{'ms min':>9}{'wall ms':>9}{'launches':>10}{'host reads':>12}")
    for group, name, fn in table:
        med, best, wall = timed(fn, a.reps)
        print(f"({group}) {name:<48}{med:>11.3f}{best:>9.3f}{wall:>9.2f}{launches(fn):>10}"
              f"{host_reads(fn):>12}")


if __name__ == "__main__":
    main()
