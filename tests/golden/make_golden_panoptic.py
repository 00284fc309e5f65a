"""Golden fixture for the panoptic evaluation, produced by the REFERENCE'S OWN code:

  * ``InstanceData`` / ``InstanceBatch`` (src/data/instance.py, imported verbatim as
    make_golden_instance.py does): the dense constructor, ``merge``, ``iou_and_size``,
    ``search_void``, ``remove_void``, ``from_list``;
  * ``PanopticSegmentationOutput`` (src/utils/output_panoptic.py, imported verbatim):
    ``weighted_instance_semantic_pred``, ``panoptic_pred``, ``superpoint_panoptic_pred``,
    ``voxel_panoptic_pred``, ``full_res_panoptic_pred``; ``scatter_mean_weighted``
    (src/utils/scatter.py);
  * ``PanopticQuality3D.compute`` (src/metrics/panoptic.py:206-381), cut out of its class with
    ``ast`` - unmodified - and run on a bare stand-in of the torchmetrics base (a namespace
    holding the two state lists and the three settings).

Stand-ins: torch_scatter / consecutive_cluster = the oracle's restatements.

Scene 1 (C = 13, stuff classes [0, 1, 2]): 37 level-1 nodes merged into 9 predicted instances,
objects with sparse ids 3k + 1:
  * instance 0 is a single node at EXACTLY half void (not void); instance 2 a single node one
    count above half (void); instance 1 holds 20 nodes;
  * several nodes of one instance overlap the same object (duplicate keys, counts summed);
  * object 1 (the floor, class 0) is overlapped by every instance;
  * void objects labelled -1 and 13;
  * instance 3 / object 7: count 2, a_size 3, b_size 3 - IoU exactly 0.5, not a TP; instance 4 /
    object 10: 1001 / 2001, just above;
  * instance 6 predicts class 0 with a small IoU: only ``pq_modified`` takes it;
  * the floor's overlap with instance 1 exceeds 2^24 (the f32 conversion rounds);
  * class 7 is seen only in predictions, classes 1 and 9 only in targets, 2, 6, 8, 10, 11, 12
    are unseen;
  * object id 2^31 - 1 in scene 1; scene 2 (5 nodes, 3 instances) reuses ids 1, 4, 7, which
    ``from_list`` shifts past 2^31.
Node logits [37, 13]: for every instance the two largest mean logits differ by more than 1e-3,
except three planted exact ties from integer logits and power-of-two sizes (the first, a middle
and the last column taking part); asserted on what the reference produced.

``big__*``: a weighted mean over groups of 1, 512, 513 and 700 rows (and an empty group).
``f64__*``: float64 evaluations of the reference's formulas on the fixture's own per-pair IoUs
and logits - the yardstick of the float bars (profiles/r19a_panoptic_errors.txt).

Usage (build container only): python tests/golden/make_golden_panoptic.py [--check]
(``--check``: regenerate and compare with the committed file array by array, bit for bit).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_instance as mgi  # noqa: E402
import make_golden_select as mgs  # noqa: E402
import make_golden_semantic_output as mso  # noqa: E402
import grid_sampling_reference as R  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

C = 13
STUFF = [0, 1, 2]
N1, NUM_INST, NV, NR = 37, 9, 150, 400
INST_SIZES = [1, 20, 1, 3, 3, 3, 2, 2, 2]
INST_CLASS = [4, 0, 5, 3, 3, 4, 0, 7, 5]
TIES = {6: (0, 5), 7: (7, 9), 8: (5, 12)}        # instance -> the two tied columns
BIG = (1 << 31) - 1                               # an object id of scene 1
# objects of scene 1: id -> label
OBJ_Y = {1: 0, 4: 1, 7: 3, 10: 3, 13: 4, 16: 5, 19: -1, 22: 13, 25: 9, 28: 4, BIG: 5}
# (instance, node of the instance, object, count)
PAIRS = [
    (0, 0, 19, 10), (0, 0, 1, 4), (0, 0, 13, 6),
    (2, 0, 22, 11), (2, 0, 1, 10),
    (3, 0, 7, 1), (3, 1, 7, 1), (3, 2, 1, 1),
    (4, 0, 10, 500), (4, 1, 10, 501), (4, 2, 1, 499), (4, 2, 7, 1),
    (5, 0, 13, 1700), (5, 1, 13, 1300), (5, 1, 10, 500), (5, 2, 1, 20),
    (6, 0, 1, 50), (6, 1, 25, 40),
    (7, 0, 1, 5), (7, 0, 28, 30), (7, 1, BIG, 7),
    (8, 0, 16, 120), (8, 1, 16, 80), (8, 1, 1, 3), (8, 0, 4, 10), (8, 1, BIG, 2),
    (1, 0, 1, (1 << 24) + 3), (1, 3, 4, 150), (1, 7, 4, 250), (1, 7, 19, 5), (1, 9, 22, 3),
    (1, 12, 28, 2),
] + [(1, k, 1, 10 + k) for k in range(1, 20)]


def cut_compute():
    code = mgs.cut("src/metrics/panoptic.py", "PanopticQuality3D", "compute")

    class Results:
        pass
    ns = {"torch": torch, "InstanceBatch": sys.modules["src.data.instance"].InstanceBatch,
          "consecutive_cluster": O.consecutive_cluster, "scatter_sum": O.scatter_sum,
          "PanopticMetricResults": Results}
    exec(compile(code, "panoptic.py", "exec"), ns)
    return ns["compute"]


FIELDS = ("pq", "sq", "rq", "pq_modified", "pq_thing", "sq_thing", "rq_thing", "pq_stuff",
          "sq_stuff", "rq_stuff", "pq_per_class", "sq_per_class", "rq_per_class",
          "precision_per_class", "recall_per_class", "tp_per_class", "fp_per_class",
          "fn_per_class", "pq_modified_per_class", "mean_precision", "mean_recall")


def f64_metrics(pair_iou, pair_gt, pair_pred, gt_counts, pred_counts, stuff, ignore):
    """The reference's formulas (src/metrics/panoptic.py:276-379) in float64 on the given f32
    per-pair IoUs."""
    pair_iou = pair_iou.double()
    is_stuff = torch.tensor([i in stuff for i in range(C)])
    has_stuff = bool(is_stuff.any())
    agrees = pair_gt == pair_pred
    gt50 = pair_iou > 0.5
    sel = agrees & gt50
    tp = torch.bincount(pair_gt[sel], minlength=C)
    iou_sum = torch.zeros(C, dtype=torch.float64).index_add_(0, pair_gt[sel], pair_iou[sel])
    sel_mod = agrees & (gt50 | is_stuff[pair_gt])
    iou_mod_sum = torch.zeros(C, dtype=torch.float64).index_add_(0, pair_gt[sel_mod],
                                                                 pair_iou[sel_mod])
    precision = tp.double() / pred_counts.double()
    precision[precision.isnan()] = 0
    recall = tp.double() / gt_counts.double()
    sq = iou_sum / tp.double()
    sq[sq.isnan()] = 0
    rq = 2 * precision * recall / (precision + recall)
    rq[rq.isnan()] = 0
    pq = sq * rq
    if has_stuff:
        den = (gt_counts + pred_counts).double() / 2
        den[is_stuff] = gt_counts[is_stuff].double()
        pq_mod = iou_mod_sum / den
    else:
        pq_mod = pq.clone()
        iou_mod_sum = iou_sum.clone()
    seen = (gt_counts + pred_counts) > 0
    default = float("nan") if ignore else 0.0
    for t in (pq, sq, rq, pq_mod, precision, recall):
        t[~seen] = default
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    out = dict(pq=pq.nanmean(), sq=sq.nanmean(), rq=rq.nanmean(), pq_modified=pq_mod.nanmean(),
               pq_thing=pq[~is_stuff].nanmean(), sq_thing=sq[~is_stuff].nanmean(),
               rq_thing=rq[~is_stuff].nanmean(),
               pq_stuff=pq[is_stuff].nanmean() if has_stuff else nan,
               sq_stuff=sq[is_stuff].nanmean() if has_stuff else nan,
               rq_stuff=rq[is_stuff].nanmean() if has_stuff else nan,
               pq_per_class=pq, sq_per_class=sq, rq_per_class=rq, precision_per_class=precision,
               recall_per_class=recall, pq_modified_per_class=pq_mod,
               mean_precision=precision.nanmean(), mean_recall=recall.nanmean(),
               iou_sum=iou_sum, iou_mod_sum=iou_mod_sum)
    return out


def scene1(rng):
    """Dense level-1 pairs, the node -> instance map, logits and node sizes."""
    inst_of_node = np.repeat(np.arange(NUM_INST), INST_SIZES)[rng.permutation(N1)]
    nodes_of = [np.where(inst_of_node == i)[0] for i in range(NUM_INST)]
    node, obj, count = [], [], []
    for i, k, o, c in PAIRS:
        node.append(nodes_of[i][k])
        obj.append(o)
        count.append(c)
    order = rng.permutation(len(node))
    node, obj, count = (np.asarray(a, dtype=np.int64)[order] for a in (node, obj, count))
    assert set(node.tolist()) == set(range(N1))
    y = np.array([OBJ_Y[o] for o in obj.tolist()], dtype=np.int64)

    logits = rng.normal(size=(N1, C)).astype(np.float32)
    node_size = rng.integers(1, 200, N1).astype(np.int64)
    for i in range(NUM_INST):
        for n in nodes_of[i]:
            logits[n, INST_CLASS[i]] += 6.0
    for i, (a, b) in TIES.items():                 # integer logits, power-of-two sizes
        n0, n1 = nodes_of[i]
        logits[[n0, n1]] = rng.integers(-3, 3, (2, C)).astype(np.float32)
        logits[n0, a], logits[n0, b] = 9.0, 5.0
        logits[n1, a], logits[n1, b] = 7.0, 9.0
        node_size[n0], node_size[n1] = 4, 8        # (9 * 4 + 7 * 8) == (5 * 4 + 9 * 8) == 92
    return inst_of_node.astype(np.int64), node, obj, count, y, logits, node_size


def build():
    torch.set_num_threads(1)
    U, csr, inst = mgi.load_reference()
    ID, IB = inst.InstanceData, inst.InstanceBatch
    sys.modules["src.data"].InstanceData = ID      # (the output's local `from src.data import`)
    scatter = importlib.import_module("src.utils.scatter")
    Output = importlib.import_module("src.utils.output_panoptic").PanopticSegmentationOutput
    Cluster = sys.modules["src.data.cluster"].Cluster
    compute = cut_compute()
    rng = np.random.default_rng(20261020)
    T = torch.from_numpy
    out = {"num_classes": np.int64(C), "stuff_classes": np.array(STUFF, dtype=np.int64)}

    idx1, node, obj, count, y, logits, node_size = scene1(rng)
    out.update(in__idx1=idx1, in__dense_node=node, in__dense_obj=obj, in__dense_count=count,
               in__dense_y=y, in__logits=logits, in__node_size=node_size)
    d1 = ID(T(node), T(obj), T(count), T(y), dense=True)
    out.update(l1_pointers=d1.pointers, l1_obj=d1.obj, l1_count=d1.count, l1_y=d1.y)
    m1 = d1.merge(T(idx1))
    out.update(m1_pointers=m1.pointers, m1_obj=m1.obj, m1_count=m1.count, m1_y=m1.y)
    assert m1.num_clusters == NUM_INST

    # scene 2: object ids that collide with scene 1's
    node2 = np.array([0, 0, 1, 2, 3, 4, 4], dtype=np.int64)
    obj2 = np.array([1, 4, 1, 4, 7, 7, 4], dtype=np.int64)
    count2 = np.array([30, 5, 12, 40, 9, 2, 6], dtype=np.int64)
    y2 = np.array([{1: 4, 4: 0, 7: 13}[o] for o in obj2.tolist()], dtype=np.int64)
    idx2 = np.array([0, 0, 1, 2, 1], dtype=np.int64)
    pred2 = np.array([4, 0, 0], dtype=np.int64)
    out.update(in__idx2=idx2, in__pred2=pred2)
    d2 = ID(T(node2), T(obj2), T(count2), T(y2), dense=True)
    out.update(l2_pointers=d2.pointers, l2_obj=d2.obj, l2_count=d2.count, l2_y=d2.y)
    m2 = d2.merge(T(idx2))
    out.update(m2_pointers=m2.pointers, m2_obj=m2.obj, m2_count=m2.count, m2_y=m2.y)

    # the reference's output object on scene 1
    ei = T(rng.integers(0, N1, (2, 60)).astype(np.int64))
    y_hist = d1.target_label_histogram(C)
    o = Output(T(logits), STUFF, torch.zeros(60), T(node_size), y_hist=y_hist, obj=d1,
               obj_edge_index=ei, obj_edge_affinity=torch.rand(60), pos=torch.zeros(N1, 3),
               obj_pos=torch.zeros(N1, 3), obj_index_pred=T(idx1))
    assert o.has_target and o.has_instance_pred
    obj_y, obj_score, obj_logits = o.weighted_instance_semantic_pred()
    score2, y2_, merged = o.panoptic_pred()
    assert torch.equal(y2_, obj_y) and torch.equal(score2, obj_score)
    for k in ("pointers", "obj", "count", "y"):
        assert torch.equal(getattr(merged, k), getattr(m1, k))
    assert obj_y.tolist() == INST_CLASS, obj_y.tolist()
    top2 = obj_logits.double().topk(2, dim=1).values
    for i in range(NUM_INST):
        gap = float(top2[i, 0] - top2[i, 1])
        if i in TIES:
            a, b = TIES[i]
            assert gap == 0.0 and float(obj_logits[i, a]) == float(obj_logits[i, b]) \
                == float(top2[i, 0]), (i, obj_logits[i])
        else:
            assert gap > 1e-3, (i, gap)
    out.update(obj_y=obj_y, obj_score=obj_score, obj_logits=obj_logits)
    sp_y, sp_index, sp_data = o.superpoint_panoptic_pred()
    out.update(sp_y=sp_y, sp_pointers=sp_data.pointers, sp_obj=sp_data.obj, sp_count=sp_data.count,
               sp_data_y=sp_data.y)

    s1 = mso.split_sizes(rng, NV, N1, {5: 60}, (0, 18, 36))
    s0 = mso.split_sizes(rng, NR, NV, {7: 90}, (0, 75, 149))
    si01, ptr1, pts1 = mso.make_hop(rng, s1)
    si_raw0, ptr0, pts0 = mso.make_hop(rng, s0)
    out.update(in__si01=si01, in__sub1_pointers=ptr1, in__sub1_points=pts1, in__si_raw0=si_raw0,
               in__sub0_pointers=ptr0, in__sub0_points=pts0)
    sub1, sub0 = Cluster(T(ptr1), T(pts1)), Cluster(T(ptr0), T(pts0))
    vox_y, vox_index, vox_data = o.voxel_panoptic_pred(super_index=T(si01))
    assert torch.equal(vox_y, o.voxel_panoptic_pred(sub=sub1)[0])
    raw_y, raw_index, raw_data = o.full_res_panoptic_pred(
        super_index_level0_to_level1=T(si01), super_index_raw_to_level0=T(si_raw0))
    assert torch.equal(raw_index, o.full_res_panoptic_pred(sub_level1_to_level0=sub1,
                                                           sub_level0_to_raw=sub0)[1])
    for tag, yy, ii, dd in (("vox", vox_y, vox_index, vox_data), ("raw", raw_y, raw_index, raw_data)):
        out.update({f"{tag}_y": yy, f"{tag}_index": ii, f"{tag}_pointers": dd.pointers,
                    f"{tag}_obj": dd.obj, f"{tag}_count": dd.count, f"{tag}_data_y": dd.y})

    # per-pair statistics, per scene and on the batch
    batch = IB.from_list([m1, m2])
    assert int(batch.obj.max()) > (1 << 31)
    pred_all = torch.cat((obj_y, T(pred2)))
    out.update(b_pointers=batch.pointers, b_obj=batch.obj, b_count=batch.count, b_y=batch.y)
    for tag, dd in (("m1", m1), ("m2", m2), ("b", batch)):
        iou, a_size, b_size = dd.iou_and_size()
        cm, pm, crop = dd.search_void(C)
        rv, keep = dd.remove_void(C)
        rv_iou = rv.iou_and_size()[0]
        assert torch.equal(keep, ~cm) and int((~pm).sum()) == rv.num_items
        out.update({f"{tag}_iou": iou, f"{tag}_a_size": a_size, f"{tag}_b_size": b_size,
                    f"{tag}_cluster_void": cm, f"{tag}_pair_void": pm, f"{tag}_cropped": crop,
                    f"{tag}_rv_iou": rv_iou, f"{tag}_rv_pointers": rv.pointers})
    cm1 = T(np.asarray(out["m1_cluster_void"]))
    assert cm1.tolist() == [i == 2 for i in range(NUM_INST)], cm1.tolist()     # half / half + 1
    iou1 = T(np.asarray(out["m1_iou"]))
    half = [(int(m1.obj[j]), float(iou1[j])) for j in range(m1.num_items) if int(m1.obj[j]) in (7, 10)]
    assert (7, 0.5) in half and any(ob == 10 and 0.5 < v < 0.5005 for ob, v in half), half
    assert int(m1.count.max()) > (1 << 24)

    # the metric
    rv, keep = batch.remove_void(C)
    pair_iou = rv.iou_and_size()[0]
    pair_gt = rv.y
    pair_pred = pred_all[keep][rv.indices]
    for tag, stuff, ignore in (("pq", STUFF, True), ("pq_all", STUFF, False), ("pq_nostuff", [], True)):
        self = types.SimpleNamespace(prediction_semantic=[obj_y, T(pred2)], instance_data=[m1, m2],
                                     num_classes=C, stuff_classes=stuff, ignore_unseen_classes=ignore)
        res = compute(self)
        for f in FIELDS:
            out[f"{tag}__{f}"] = torch.as_tensor(getattr(res, f))
        gt_counts = res.tp_per_class + res.fn_per_class
        pred_counts = res.tp_per_class + res.fp_per_class
        out[f"{tag}__gt_count"], out[f"{tag}__pred_count"] = gt_counts, pred_counts
        for k, v in f64_metrics(pair_iou, pair_gt, pair_pred, gt_counts, pred_counts, stuff,
                                ignore).items():
            out[f"f64__{tag}__{k}"] = v
    t = out["pq__tp_per_class"]
    seen = (out["pq__gt_count"] + out["pq__pred_count"]) > 0
    assert seen.tolist() == [c in (0, 1, 3, 4, 5, 7, 9) for c in range(C)], seen.tolist()
    assert int(out["pq__gt_count"][7]) == 0 and int(out["pq__pred_count"][9]) == 0
    assert int(t[3]) == 1 and int(t[0]) >= 1, t.tolist()         # 0.5 exactly is no TP
    assert float(out["f64__pq__iou_mod_sum"][0]) > float(out["f64__pq__iou_sum"][0])

    # weighted means past the sequential limit
    sizes = [1, 512, 513, 700, 0, 3]
    idx_big = np.repeat(np.arange(len(sizes)), sizes)
    idx_big = idx_big[rng.permutation(idx_big.size)].astype(np.int64)
    x_big = rng.normal(size=(idx_big.size, C)).astype(np.float32)
    w_big = rng.integers(0, 300, idx_big.size).astype(np.int64)
    ref_big = scatter.scatter_mean_weighted(T(x_big), T(idx_big), T(w_big), dim_size=len(sizes))
    out.update(big__in__x=x_big, big__in__idx=idx_big, big__in__w=w_big, big__mean=ref_big)
    wd = T(w_big).float().double().view(-1, 1)
    num = torch.zeros(len(sizes), C, dtype=torch.float64).index_add_(0, T(idx_big), T(x_big).double() * wd)
    den = torch.zeros(len(sizes), dtype=torch.float64).index_add_(0, T(idx_big), wd.view(-1))
    den[den == 0] = 1
    out["f64__big__mean"] = num / den.view(-1, 1)
    out["f64__big__score"] = out["f64__big__mean"].softmax(dim=1).max(dim=1).values
    out["big__score"] = ref_big.softmax(dim=1).max(dim=1).values
    w1 = T(node_size).float().double().view(-1, 1)
    num = torch.zeros(NUM_INST, C, dtype=torch.float64).index_add_(0, T(idx1), T(logits).double() * w1)
    den = torch.zeros(NUM_INST, dtype=torch.float64).index_add_(0, T(idx1), w1.view(-1))
    out["f64__obj_logits"] = num / den.view(-1, 1)
    out["f64__obj_score"] = out["f64__obj_logits"].softmax(dim=1).max(dim=1).values
    return out


def main():
    out = build()
    path = os.path.join(HERE, "panoptic.npz")
    if "--check" in sys.argv:
        old = dict(np.load(path))
        assert set(old) == set(out), sorted(set(old) ^ set(out))
        for k, v in out.items():
            v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            assert R.bits_equal(old[k], v), f"{k} differs from the committed fixture"
        print(f"panoptic.npz: {len(out)} arrays bit-identical to the regenerated ones")
        return
    mg.save("panoptic.npz", **out)
    print(f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
