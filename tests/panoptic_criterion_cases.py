"""The comparisons of the panoptic criterion against tests/golden/panoptic_criterion.npz (written
by tests/golden/make_golden_panoptic_criterion.py from the reference's own code), shared by the
CPU route's tests and the device's: every function takes the device to run on.

Everything integer - major objects, void masks, keep masks, cases, tp / fp / tn / fn - is
compared exactly.  Losses and gradients fall under ``panoptic_cases.bar`` / ``within``: the
yardstick is the fixture's float64 evaluation ``f64__*``, the bar per element 4 x the reference's
own f32 deviation from it and never below one f32 ulp of the value.  The measured deviations are
in profiles/r20a_panoptic_criterion_errors.txt."""
import functools

import numpy as np
import torch

import panoptic_cases as pc
from conftest import load_golden

C = 13
SETTINGS = {"plain": (False, None), "w1": (True, [1, 1, 1, 1]), "w2": (True, [0.5, 4, 0, 2])}
POS_WEIGHTS = {"pw1": 1.0, "pw25": 2.5}
LAMBDA = 10


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("panoptic_criterion.npz")


def T(key, dev="cpu"):
    return torch.from_numpy(np.asarray(golden()[key])).to(dev)


def instance(tag, dev):
    from superpoint_transformer_amd.instance import InstanceData
    return InstanceData(*(T(f"{tag}_{k}", dev) for k in ("pointers", "obj", "count", "y")))


def same_major(got, tag):
    for t, k in zip(got, ("obj", "count", "y")):
        assert t.dtype == torch.int64
        assert torch.equal(t.cpu(), T(f"{tag}_major_{k}")), (tag, k)


# ---- major objects -------------------------------------------------------------------------------
def check_major(dev):
    from superpoint_transformer_amd import panoptic
    for tag in ("a", "b"):
        d = instance(tag, dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        got = panoptic.major_objects(d, C, status=status)
        same_major(got, tag)
        same_major(panoptic.major_objects(d, C, check=False), tag)
        assert status.tolist() == [0, 0]
        if torch.device(dev).type != "cpu":                  # the yardstick on the device agrees
            for a, b in zip(got, d.major(C)):
                assert torch.equal(a, b)
    panoptic.verify_major(block=True)
    # scene A took the global branch (its at-half clusters moved every void-major cluster), scene
    # B did not: the same planted cluster differs between the two
    assert T("a_major_y")[3].item() == 0 and T("b_major_y")[2].item() == 13
    d = instance("c", dev)
    obj, _, y = panoptic.major_objects(d, C)
    assert torch.equal(obj.cpu(), T("c_major_obj")) and torch.equal(y.cpu(), T("c_major_y"))


def check_empty_cluster(dev):
    """A cluster without a pair: the reference indexes out of range; here a status and a refusal."""
    import pytest
    from superpoint_transformer_amd import panoptic
    from superpoint_transformer_amd.instance import InstanceData
    d = InstanceData(torch.tensor([0, 2, 2, 3]), torch.tensor([4, 7, 1]), torch.tensor([5, 9, 2]),
                     torch.tensor([0, 13, 1])).to(dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    obj, count, y = panoptic.major_objects(d, C, check=False, status=status)
    assert status.tolist() == [1, 0]
    assert obj.tolist() == [7, -1, 1] and count.tolist() == [9, 0, 2] and y.tolist() == [13, -1, 1]
    with pytest.raises(ValueError, match="without a pair"):
        panoptic.major_objects(d, C, check=True)
        panoptic.verify_major(block=True)


# ---- the loss ------------------------------------------------------------------------------------
def inputs(tag, dev):
    from superpoint_transformer_amd import panoptic, predict
    d = instance(tag, dev)
    hist = T("c_y_hist1" if tag == "c" else "d_y_hist", dev).long()
    obj, _, y = panoptic.major_objects(d, C)
    return dict(d=d, hist=hist, void=predict.void_mask(hist), obj=obj, y=y,
                ei=T(f"{tag}_edge_index", dev), target=T(f"{tag}_target", dev),
                logits=T(f"{tag}_logits", dev))


def check_masks_and_cases(dev):
    from superpoint_transformer_amd import ops
    a = inputs("c", dev)
    assert torch.equal(a["void"].cpu(), T("c_void"))
    keep = T("c_keep")
    # the cases through the loss itself: with a one-hot table, logits 0 and targets 0 every edge
    # of the case - and no other - gets the gradient 0.5 / (edges of the case)
    zeros = torch.zeros_like(a["logits"])
    for kind in range(4):
        table = [float(k == kind) for k in range(4)]
        x = zeros.clone().requires_grad_()
        loss = ops.edge_affinity_loss(x, zeros, a["ei"], a["void"], a["obj"], a["y"],
                                      case_weights=table)
        grad = torch.autograd.grad(loss, x)[0].cpu()
        member = keep & (T("c_kind") == kind)
        assert int(member.sum()) > 0
        assert torch.equal(grad != 0, member), kind
        assert torch.equal(grad[member], torch.full_like(grad[member], 0.5 / int(member.sum())))
        assert abs(float(loss.detach()) - np.log(2.0)) < 1e-6
    assert int(T("c_stats").sum()) == int(keep.sum())


def criterion(sname, pname):
    from superpoint_transformer_amd.criterion import EdgeAffinityCriterion
    weighted, cw = SETTINGS[sname]
    return EdgeAffinityCriterion(weighted=weighted, case_weights=cw, pos_weight=POS_WEIGHTS[pname])


def run_setting(a, sname, pname, dev):
    crit = criterion(sname, pname).to(dev)
    x = a["logits"].clone().requires_grad_()
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    loss = crit(x, a["target"], a["ei"], a["void"], a["obj"], a["y"], stats=stats)
    grad = torch.autograd.grad(loss, x)[0]
    return loss.detach(), grad, stats


def check_losses(dev):
    """Every setting of scene C; returns {name: (our deviation, the reference's)}."""
    g = golden()
    a = inputs("c", dev)
    report = {}
    for sname in SETTINGS:
        for pname in POS_WEIGHTS:
            key = f"{sname}_{pname}"
            loss, grad, stats = run_setting(a, sname, pname, dev)
            assert loss.dtype == torch.float32 and grad.dtype == torch.float32
            assert stats.tolist() == T("c_stats").tolist(), key
            report[f"{key} loss"] = pc.within(loss, g[f"c__{key}_loss"], g[f"f64__c__{key}_loss"],
                                              f"{key} loss")
            report[f"{key} grad"] = pc.within(grad, g[f"c__{key}_grad"], g[f"f64__c__{key}_grad"],
                                              f"{key} grad")
            assert not bool(grad.cpu()[~T("c_keep")].any()), key     # dropped edges: exact zeros
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    # a table that is not of length 4 means no weighting, like None
    from superpoint_transformer_amd.criterion import EdgeAffinityCriterion
    plain = run_setting(a, "plain", "pw1", dev)
    for cw in (None, [1.0, 2.0, 3.0]):
        crit = EdgeAffinityCriterion(weighted=True, case_weights=cw).to(dev)
        x = a["logits"].clone().requires_grad_()
        assert pc.bits(crit(x, a["target"], a["ei"], a["void"], a["obj"], a["y"])) == pc.bits(plain[0])
    return report


def output_of(a, dev):
    from superpoint_transformer_amd.output import PanopticSegmentationOutput
    n = a["hist"].shape[0]
    return PanopticSegmentationOutput(
        torch.zeros(n, C, device=dev), [], a["logits"].clone().requires_grad_(),
        torch.ones(n, dtype=torch.long, device=dev), y_hist=a["hist"], obj=a["d"],
        obj_edge_index=a["ei"], obj_edge_affinity=a["target"], pos=torch.zeros(n, 3, device=dev),
        obj_pos=torch.zeros(n, 3, device=dev))


def check_output_route(dev):
    """The criterion on a ``PanopticSegmentationOutput`` with a target: the bits of the tensor
    route; without a target: a refusal."""
    import pytest
    a = inputs("c", dev)
    crit = criterion("w2", "pw25").to(dev)
    o = output_of(a, dev)
    loss = crit(o)
    grad = torch.autograd.grad(loss, o.edge_affinity_logits)[0]
    want = run_setting(a, "w2", "pw25", dev)
    assert pc.bits(loss) == pc.bits(want[0]) and pc.bits(grad) == pc.bits(want[1])
    o.obj_pos = None
    with pytest.raises(ValueError, match="no target"):
        crit(o)


def check_combined(dev):
    """``semantic + 10 * edge affinity`` of ``model_step`` through ``PanopticCriterion``."""
    from superpoint_transformer_amd.criterion import (EdgeAffinityCriterion, PanopticCriterion,
                                                       SemanticCriterion)
    g = golden()
    a = inputs("c", dev)
    crit = PanopticCriterion(SemanticCriterion(C, "ce_kl", lambdas=(1, 50)), EdgeAffinityCriterion(),
                             edge_affinity_loss_lambda=LAMBDA).to(dev)
    sem = [T("c_sem1", dev), T("c_sem2", dev)]
    hists = [a["hist"], T("c_y_hist2", dev).long()]
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    confmat = torch.zeros(C, C, dtype=torch.int64, device=dev)
    loss, semantic, edge = crit(sem, hists, a["logits"], a["target"], a["ei"], a["void"], a["obj"],
                                a["y"], confmat=confmat, stats=stats)
    assert stats.tolist() == T("c_stats").tolist()
    assert int(confmat.sum()) == int(hists[0][:, :C].sum())
    assert pc.bits(edge) == pc.bits(run_setting(a, "plain", "pw1", dev)[0])
    report = {"semantic": pc.within(semantic, g["c__semantic"], g["f64__c__semantic"], "semantic"),
              "combined": pc.within(loss, g["c__combined"], g["f64__c__combined"], "combined")}
    return report


def check_all_void(dev):
    """Case D: every edge joins two void nodes - NaN loss (the mean of nothing), zero gradient."""
    g = golden()
    a = inputs("d", dev)
    assert a["void"].tolist() == [True, True, True, False]
    for sname in SETTINGS:                                   # (the reference: plain only, its
        for pname in POS_WEIGHTS:                            # weighted loss asserts on no edge)
            loss, grad, stats = run_setting(a, sname, pname, dev)
            assert bool(torch.isnan(loss)) and grad.shape == (5,) and not bool(grad.any())
            assert stats.tolist() == [0, 0, 0, 0]
            if sname == "plain":
                assert np.isnan(g[f"d__plain_{pname}_loss"]) and not g[f"d__plain_{pname}_grad"].any()


def check_no_edge(dev):
    """E = 0, decided from the shape: NaN and an empty gradient, like the mean of an empty tensor."""
    a = inputs("d", dev)
    x = torch.zeros(0, device=dev, requires_grad=True)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    loss = criterion("w2", "pw25").to(dev)(x, torch.zeros(0, device=dev),
                                          torch.zeros(2, 0, dtype=torch.long, device=dev),
                                          a["void"], a["obj"], a["y"], stats=stats)
    assert bool(torch.isnan(loss)) and torch.autograd.grad(loss, x)[0].shape == (0,)
    assert stats.tolist() == [0, 0, 0, 0]


def check_extreme_logits(dev):
    """Logits of +-90 (and the largest f32) under every target: finite loss and gradient."""
    a = inputs("c", dev)
    x = a["logits"].clone()
    x[0::4], x[1::4], x[2::4] = 90.0, -90.0, 3.0e38
    x[3::8] = -3.0e38
    for sname in ("plain", "w2"):
        crit = criterion(sname, "pw25").to(dev)
        leaf = x.clone().requires_grad_()
        loss = crit(leaf, a["target"], a["ei"], a["void"], a["obj"], a["y"])
        grad = torch.autograd.grad(loss, leaf)[0]
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())


def check_metric(dev):
    from superpoint_transformer_amd.metrics import BinaryEdgeStats
    a = inputs("c", dev)
    m = BinaryEdgeStats(device=dev)
    assert m.oa() == 0.0 and m.f1() == 0.0                   # 0 / 0
    m.update(a["logits"], a["target"], a["ei"], a["void"])
    tp, fp, tn, fn = T("c_stats").tolist()
    assert m.compute() == (tp, fp, tn, fn)
    assert m.oa() == (tp + tn) / (tp + fp + tn + fn) and m.f1() == 2 * tp / (2 * tp + fp + fn)
    m.update(a["logits"], a["target"], a["ei"], a["void"])
    assert m.compute() == (2 * tp, 2 * fp, 2 * tn, 2 * fn)
    m.reset()
    assert m.compute() == (0, 0, 0, 0)


def random_case(g, per_cluster, e, seed, dev):
    """Seeded instance of ``g`` clusters, a histogram making about a fifth of the nodes void,
    ``e`` edges with some ends out of range, targets and logits."""
    d = pc.random_instance(g, per_cluster, C, seed)
    rng = np.random.default_rng(seed + 1)
    hist = torch.from_numpy(rng.integers(0, 20, (g, C + 1)))
    hist[:, C] = torch.from_numpy(np.where(rng.random(g) < 0.2, 400, 0))
    ei = torch.from_numpy(rng.integers(0, g, (2, e)))
    target = torch.from_numpy(rng.choice([0.0, 1.0, 0.5, 0.3], e).astype(np.float32))
    logits = torch.from_numpy((rng.normal(size=e) * 3).astype(np.float32))
    return d.to(dev), hist.to(dev), ei.to(dev), target.to(dev), logits.to(dev)
