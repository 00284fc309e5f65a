"""The comparisons of the panoptic evaluation against tests/golden/panoptic.npz (written by
tests/golden/make_golden_panoptic.py from the reference's own code), shared by the CPU route's
tests and the device's: every function takes the device to run on.

Exact items are compared exactly (``torch.equal``; f32 IoUs and short weighted means byte for
byte).  Float bars (``bar``): the yardstick is the fixture's float64 evaluation ``f64__*``; the
bar of a quantity is 4 x the reference's own f32 deviation from it and never below one f32 ulp of
the value - the project's standing margin.  The measured deviations of the reference and of the
device, per quantity, are in profiles/r19a_panoptic_errors.txt."""
import functools

import numpy as np
import torch

from conftest import load_golden
from superpoint_transformer_amd import panoptic  # noqa: F401  (the feature under test)

C = 13
STUFF = [0, 1, 2]
SCALARS = ("pq", "sq", "rq", "pq_modified", "pq_thing", "sq_thing", "rq_thing", "pq_stuff",
           "sq_stuff", "rq_stuff", "mean_precision", "mean_recall")
PER_CLASS = ("pq_per_class", "sq_per_class", "rq_per_class", "precision_per_class",
             "recall_per_class", "pq_modified_per_class")
VARIANTS = {"pq": (STUFF, True), "pq_all": (STUFF, False), "pq_nostuff": (None, True)}


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("panoptic.npz")


def T(key, dev="cpu"):
    return torch.from_numpy(np.asarray(golden()[key])).to(dev)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def instance(tag, dev):
    from superpoint_transformer_amd.instance import InstanceData
    return InstanceData(*(T(f"{tag}_{k}", dev) for k in ("pointers", "obj", "count", "y")))


def same_instance(d, tag):
    for k in ("pointers", "obj", "count", "y"):
        assert torch.equal(getattr(d, k).cpu(), T(f"{tag}_{k}")), (tag, k)


def bar(ref, f64):
    """Per element: max(4 |ref - f64|, one f32 ulp of |f64|)."""
    ref, f64 = np.asarray(ref, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    ulp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.maximum(4 * np.abs(ref - f64), ulp)


def within(got, ref, f64, what):
    """NaNs where the yardstick has them, everything else within the bar; returns the largest
    deviation of ``got`` and of ``ref`` from the yardstick."""
    got = np.asarray(torch.as_tensor(got).detach().cpu().double().numpy())
    ref, f64 = np.asarray(ref, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    assert got.shape == f64.shape, (what, got.shape, f64.shape)
    nan = np.isnan(f64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ: {got} vs {f64}"
    dev_got = np.where(nan, 0.0, np.abs(got - f64))
    dev_ref = np.where(nan, 0.0, np.abs(ref - f64))
    limit = np.where(nan, 0.0, bar(ref, f64))
    print(f"{what}: deviation {dev_got.max():.3e} (reference {dev_ref.max():.3e}, "
          f"bar there {np.asarray(limit).flat[int(dev_got.argmax())]:.3e})")
    assert (dev_got <= limit).all(), f"{what}: {dev_got} above {limit}"
    return float(dev_got.max()), float(dev_ref.max())


# ---- merge ---------------------------------------------------------------------------------------
def check_merge(dev):
    from superpoint_transformer_amd import panoptic
    for scene in ("1", "2"):
        d = instance(f"l{scene}", dev)
        idx = T(f"in__idx{scene}", dev)
        m = panoptic.merge_instances(d, idx)
        same_instance(m, f"m{scene}")
        same_instance(panoptic.merge_instances(d, idx, num_parents=m.num_groups), f"m{scene}")
        if torch.device(dev).type != "cpu":                  # the existing composition agrees
            old = d.merge(idx)
            for k in ("pointers", "obj", "count", "y"):
                assert torch.equal(getattr(old, k), getattr(m, k))


def batch(dev):
    from superpoint_transformer_amd.instance import InstanceData
    b = InstanceData.from_list([instance("m1", dev), instance("m2", dev)])
    same_instance(b, "b")
    return b


# ---- pair statistics -----------------------------------------------------------------------------
def check_stats(dev):
    from superpoint_transformer_amd import panoptic
    for tag in ("m1", "m2", "b"):
        d = instance(tag, dev)
        s = panoptic.pair_stats(d, C)
        assert torch.equal(s.a_size.cpu(), T(f"{tag}_a_size")), tag
        assert torch.equal(s.b_size.cpu(), T(f"{tag}_b_size")), tag
        assert bits(s.iou) == bits(T(f"{tag}_iou")), tag
        assert torch.equal(s.is_cluster_void.cpu(), T(f"{tag}_cluster_void")), tag
        assert torch.equal(s.is_pair_void.cpu(), T(f"{tag}_pair_void")), tag
        assert torch.equal(s.pair_cropped_count.cpu(), T(f"{tag}_cropped")), tag
        keep = ~s.is_pair_void.cpu()
        assert bits(s.kept_iou.cpu()[keep]) == bits(T(f"{tag}_rv_iou")), tag
        assert not s.kept_iou.cpu()[~keep].any()
        # one head per object that keeps a pair, on its last kept pair
        obj = d.obj.cpu()
        heads = s.gt_head.cpu()
        assert not (heads & ~keep).any()
        assert sorted(obj[heads].tolist()) == sorted(set(obj[keep].tolist()))
        for j in torch.where(heads)[0].tolist():
            later = (obj[j + 1:] == obj[j]) & keep[j + 1:]
            assert not later.any()
        assert s.status.tolist() == [0, 0, 0, 0]
    # a count past 2^24 rounds in the conversion, and the IoU shows it
    d = instance("m1", "cpu")
    j = int(d.count.argmax())
    assert int(d.count[j]) > (1 << 24) and int(d.count[j].float()) != int(d.count[j])
    # with a pair_cropped_count on the data, b_size takes it
    d = instance("m1", dev)
    d.pair_cropped_count = torch.arange(d.num_items, device=dev)
    s = panoptic.pair_stats(d, C)
    assert torch.equal(s.b_size.cpu(), T("m1_b_size") + torch.arange(d.num_items))
    if torch.device(dev).type != "cpu":                      # the existing composition agrees
        iou, a_size, b_size = d.iou_and_size()
        assert bits(iou) == bits(s.iou) and torch.equal(b_size, s.b_size)


# ---- the output object ---------------------------------------------------------------------------
def output(dev, with_target=True, **kw):
    from superpoint_transformer_amd.output import PanopticSegmentationOutput
    n = T("in__logits").shape[0]
    args = dict(obj_index_pred=T("in__idx1", dev))
    if with_target:
        d = instance("l1", dev)
        y = d.y.clone()
        y[(y < 0) | (y > C)] = C
        y_hist = torch.zeros(d.num_groups, C + 1, dtype=torch.long, device=dev)
        y_hist.index_put_((d.indices, y), d.count, accumulate=True)
        args.update(y_hist=y_hist, obj=d,
                    obj_edge_index=torch.zeros(2, 4, dtype=torch.long, device=dev),
                    obj_edge_affinity=torch.zeros(4, device=dev), pos=torch.zeros(n, 3, device=dev),
                    obj_pos=torch.zeros(n, 3, device=dev))
    args.update(kw)
    return PanopticSegmentationOutput(T("in__logits", dev), STUFF, torch.zeros(4, device=dev),
                                      T("in__node_size", dev), **args)


def check_output(dev):
    from superpoint_transformer_amd.data import Cluster
    o = output(dev)
    assert o.has_target and o.has_instance_pred and not o.has_multi_instance_pred
    obj_y, obj_score, obj_logits = o.weighted_instance_semantic_pred()
    assert torch.equal(obj_y.cpu(), T("obj_y"))
    assert bits(obj_logits) == bits(T("obj_logits"))          # groups below the sequential limit
    within(obj_score, golden()["obj_score"], golden()["f64__obj_score"], "obj_score")
    score, y, m = o.panoptic_pred()
    assert torch.equal(y.cpu(), T("obj_y")) and bits(score) == bits(obj_score)
    same_instance(m, "m1")
    sp_y, sp_index, sp = o.superpoint_panoptic_pred()
    assert torch.equal(sp_y.cpu(), T("sp_y")) and sp_index is o.obj_index_pred
    for k, name in (("pointers", "sp_pointers"), ("obj", "sp_obj"), ("count", "sp_count"),
                    ("y", "sp_data_y")):
        assert torch.equal(getattr(sp, k).cpu(), T(name)), name
    sub1 = Cluster(T("in__sub1_pointers", dev), T("in__sub1_points", dev))
    sub0 = Cluster(T("in__sub0_pointers", dev), T("in__sub0_points", dev))
    si01, si_raw0 = T("in__si01", dev), T("in__si_raw0", dev)

    def same(res, tag):
        yy, ii, dd = res
        assert torch.equal(yy.cpu(), T(f"{tag}_y")) and torch.equal(ii.cpu(), T(f"{tag}_index")), tag
        for k, name in (("pointers", f"{tag}_pointers"), ("obj", f"{tag}_obj"),
                        ("count", f"{tag}_count"), ("y", f"{tag}_data_y")):
            assert torch.equal(getattr(dd, k).cpu(), T(name)), name
    same(o.voxel_panoptic_pred(super_index=si01), "vox")
    same(o.voxel_panoptic_pred(sub=sub1), "vox")
    for kw in (dict(super_index_level0_to_level1=si01, super_index_raw_to_level0=si_raw0),
               dict(sub_level1_to_level0=sub1, sub_level0_to_raw=sub0),
               dict(super_index_level0_to_level1=si01, sub_level0_to_raw=sub0),
               dict(sub_level1_to_level0=sub1, super_index_raw_to_level0=si_raw0)):
        same(o.full_res_panoptic_pred(**kw), "raw")
    # thin parts
    assert bits(o.edge_affinity_pred) == bits(o.edge_affinity_logits.sigmoid())
    assert o.void_edge_mask.shape == (4,)
    if torch.device(dev).type != "cpu":                      # (InstanceData.major: device only)
        assert len(o.sanitized_edge_affinities()) == 4
    # without a target: no instance data; without a prediction: nothing
    o2 = output(dev, with_target=False)
    score, y, m = o2.panoptic_pred()
    assert m is None and torch.equal(y.cpu(), T("obj_y")) and o2.void_edge_mask is None
    o3 = output(dev, obj_index_pred=None)
    assert o3.panoptic_pred() == (None, None, None)
    assert o3.weighted_instance_semantic_pred() == (None, None, None)


def check_big_mean(dev):
    """Groups of 1, 512, 513, 700, 0 and 3 rows: bit for bit up to the sequential limit, within
    the bar past it."""
    from superpoint_transformer_amd import panoptic
    assert panoptic.SEQUENTIAL_ROWS == 512
    x, idx, w = T("big__in__x", dev), T("big__in__idx", dev), T("big__in__w", dev)
    got = panoptic.weighted_group_mean(x, idx, w, 6)
    ref, f64 = golden()["big__mean"], golden()["f64__big__mean"]
    sizes = torch.bincount(idx.cpu(), minlength=6).tolist()
    assert sizes == [1, 512, 513, 700, 0, 3]
    for g, n in enumerate(sizes):
        if n <= panoptic.SEQUENTIAL_ROWS or torch.device(dev).type == "cpu":
            assert bits(got[g]) == bits(torch.from_numpy(ref[g])), (g, n)
    assert not got[4].any()                                   # no row: 0 / 1
    dev_got, dev_ref = within(got, ref, f64, "obj_logits past the sequential limit")
    score = panoptic.semantic_score(got)
    dev_s, ref_s = within(score, golden()["big__score"], golden()["f64__big__score"], "obj_score")
    return {"obj_logits": (dev_got, dev_ref), "obj_score": (dev_s, ref_s)}


# ---- the metric ----------------------------------------------------------------------------------
def metric(dev, variant, one_update):
    from superpoint_transformer_amd.metrics import PanopticQuality3D
    stuff, ignore = VARIANTS[variant]
    pq = PanopticQuality3D(C, ignore_unseen_classes=ignore, stuff_classes=stuff, device=dev)
    m1, m2 = instance("m1", dev), instance("m2", dev)
    p1, p2 = T("obj_y", dev), T("in__pred2", dev)
    if one_update:
        pq.update(torch.cat((p1, p2)), batch(dev))
    else:
        pq.update(p1, m1)
        pq.update(p2, m2)
    return pq


def check_metric(dev, variant):
    g = golden()
    results, report = [], {}
    for one_update in (False, True):
        pq = metric(dev, variant, one_update)
        assert torch.equal(pq.tp.cpu(), T(f"{variant}__tp_per_class"))
        assert torch.equal(pq.gt_count.cpu(), T(f"{variant}__gt_count"))
        assert torch.equal(pq.pred_count.cpu(), T(f"{variant}__pred_count"))
        res = pq.compute()
        assert torch.equal(res.tp_per_class, T(f"{variant}__tp_per_class"))
        assert torch.equal(res.fp_per_class, T(f"{variant}__fp_per_class"))
        assert torch.equal(res.fn_per_class, T(f"{variant}__fn_per_class"))
        # the reference's f32 sums are not among its results (SQ and PQ-modified, below, carry
        # them): the two sums are held to the floor of the bar, one f32 ulp of the value
        for name, got in (("iou_sum", pq.iou_sum), ("iou_mod_sum", pq.iou_mod_sum)):
            f64 = g[f"f64__{variant}__{name}"]
            report[name] = within(got, f64, f64, f"{variant} {name}")
        for f in SCALARS + PER_CLASS:
            report[f] = within(getattr(res, f), g[f"{variant}__{f}"], g[f"f64__{variant}__{f}"],
                               f"{variant} {f}")
        results.append((bits(pq.state), [bits(getattr(res, f)) for f in SCALARS + PER_CLASS]))
        pq.reset()
        assert not pq.state.any() and not pq.status.any()
    return results, report


# ---- shapes --------------------------------------------------------------------------------------
def random_instance(g, per_cluster, c, seed, spread=1):
    """A CSR of ``g`` clusters with ``per_cluster`` distinct objects each; object ids 3k + 1
    times ``spread``; object labels in [-1, c], so some are void."""
    from superpoint_transformer_amd.instance import InstanceData
    rng = np.random.default_rng(seed)
    n_obj = max(per_cluster + 10, g // 3)
    obj_y = rng.integers(-1, c + 1, n_obj)
    obj = np.concatenate([rng.permutation(n_obj)[:per_cluster] for _ in range(g)])
    count = rng.integers(1, 50, obj.size)
    count[rng.integers(0, obj.size)] = (1 << 24) + 1
    ptr = np.arange(g + 1) * per_cluster
    T = torch.from_numpy
    return InstanceData(T(ptr), T((obj * 3 + 1) * spread), T(count), T(obj_y[obj]))
