"""The panoptic criterion on the device - the kernels behind ``panoptic.major_objects`` and
``ops.edge_affinity_loss`` - against the reference's own output (tests/golden/
panoptic_criterion.npz, the comparisons of tests/panoptic_criterion_cases.py that the CPU route
passes in tests/test_panoptic_criterion_reference_cpu.py), against the CPU route on seeded
instances, run to run, under graph capture, and inside ``hotpath.SPTPanopticStep``.

Float bars.  Fixture: ``panoptic_cases.bar``.  Device against the CPU route: both evaluate every
term and every gradient entry in float64 and round to f32 once, so they may differ by the one
rounding - one f32 ulp of the value per element."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc
import panoptic_criterion_cases as cc

pytestmark = pytest.mark.gpu


def test_major_objects_equal_the_reference(dev):
    cc.check_major(dev)


def test_a_cluster_without_a_pair_is_refused(dev):
    cc.check_empty_cluster(dev)


def test_void_masks_and_edge_cases_are_exact(dev):
    cc.check_masks_and_cases(dev)


def test_losses_gradients_and_counters_in_every_setting(dev):
    cc.check_losses(dev)


def test_criterion_on_an_output_object(dev):
    cc.check_output_route(dev)


def test_combined_loss_of_model_step(dev):
    cc.check_combined(dev)


def test_all_void_edges_give_nan_and_a_zero_gradient(dev):
    cc.check_all_void(dev)


def test_no_edge_at_all(dev):
    cc.check_no_edge(dev)


def test_extreme_logits_stay_finite(dev):
    cc.check_extreme_logits(dev)


def test_binary_edge_stats(dev):
    cc.check_metric(dev)


def one_ulp(got, want, what):
    got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)
    print(f"{what}: largest deviation {err.max():.3e} ({(err / ulp).max():.2f} ulp)")
    assert (err <= ulp).all(), what


# clusters x pairs per cluster x edges: one of each; more than one workgroup of clusters; a
# cluster past a wave's worth of pairs (65, 70: the wave search) next to the lane search (64);
# edge counts around the workgroup (255 / 256 / 257) and the largest sizes asked for
RANDOM = [(1, 1, 1), (300, 3, 255), (700, 64, 256), (17, 65, 257), (40, 70, 1000), (2000, 2, 5000)]


@pytest.mark.parametrize("g,per_cluster,e", RANDOM)
def test_seeded_instances_against_the_cpu_route(g, per_cluster, e, dev):
    from superpoint_transformer_amd import ops, panoptic, predict
    d, hist, ei, target, logits = cc.random_case(g, per_cluster, e, seed=g + e, dev="cpu")
    if e > 10:
        ei[0, 3], ei[1, 7] = g, -1                           # out of range: dropped and counted
    got_major = panoptic.major_objects(d.to(dev), cc.C)
    want_major = panoptic.major_objects(d, cc.C)
    for a, b, c in zip(got_major, want_major, d.to(dev).major(cc.C)):
        assert torch.equal(a.cpu(), b) and torch.equal(a, c)
    panoptic.verify_major(block=True)
    void = predict.void_mask(hist.to(dev))
    assert torch.equal(void.cpu(), predict.void_mask(hist))
    for cw, pw in ((None, None), ([0.5, 4, 0, 2], 2.5)):
        res = []
        for where in ("cpu", dev):
            x = logits.to(where).requires_grad_()
            stats = torch.zeros(4, dtype=torch.int64, device=where)
            status = torch.zeros(1, dtype=torch.int32, device=where)
            loss = ops.edge_affinity_loss(
                x, target.to(where), ei.to(where), predict.void_mask(hist.to(where)),
                want_major[0].to(where), want_major[2].to(where), case_weights=cw, pos_weight=pw,
                stats=stats, status=status)
            grad = torch.autograd.grad(loss, x)[0]
            res.append((loss.detach(), grad, stats.cpu(), status.cpu()))
        (l0, g0, s0, t0), (l1, g1, s1, t1) = res
        assert torch.equal(s0, s1) and torch.equal(t0, t1)
        assert t0.tolist() == [2 if e > 10 else 0]
        assert torch.equal(torch.isnan(l0), torch.isnan(l1.cpu()))
        if not bool(torch.isnan(l0)):
            one_ulp(l1, l0, "loss")
            one_ulp(g1, g0, "gradient")


def test_loss_and_gradient_are_bitwise_reproducible(dev):
    a = cc.inputs("c", dev)
    first = cc.run_setting(a, "w2", "pw25", dev)
    d, hist, ei, target, logits = cc.random_case(2000, 2, 5000, seed=11, dev=dev)
    from superpoint_transformer_amd import ops, panoptic, predict
    obj, _, y = panoptic.major_objects(d, cc.C)
    void = predict.void_mask(hist)

    def big():
        x = logits.clone().requires_grad_()
        loss = ops.edge_affinity_loss(x, target, ei, void, obj, y, case_weights=[0.5, 4, 0, 2])
        return pc.bits(loss), pc.bits(torch.autograd.grad(loss, x)[0])
    big0 = big()
    for _ in range(3):
        again = cc.run_setting(a, "w2", "pw25", dev)
        assert pc.bits(again[0]) == pc.bits(first[0]) and pc.bits(again[1]) == pc.bits(first[1])
        assert big() == big0


def test_criterion_is_capturable_and_replays_the_eager_loss(dev):
    """Major objects, the weighted loss with its counters, and the backward inside
    torch.cuda.graph: a host synchronisation inside a capture raises, so capturing at all is the
    property the reference's ``torch.where`` / ``bool(...)`` composition cannot have.  Replays
    give the eager bits."""
    from superpoint_transformer_amd import panoptic
    a = cc.inputs("c", dev)
    crit = cc.criterion("w2", "pw25").to(dev)

    def run(x, stats):
        obj, _, y = panoptic.major_objects(a["d"], cc.C)
        return crit(x, a["target"], a["ei"], a["void"], obj, y, stats=stats)
    b = a["logits"].clone().requires_grad_()
    eager = run(b, torch.zeros(4, dtype=torch.int64, device=dev))
    eg = torch.autograd.grad(eager, b)[0].clone()
    eager = eager.detach().clone()
    del b
    x = a["logits"].clone().requires_grad_()
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                  # warm-up: allocator, workspace
            torch.autograd.grad(run(x, stats), x)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        loss = run(x, stats)
        grad = torch.autograd.grad(loss, x)[0]
    for _ in range(2):
        loss.detach().fill_(float("nan"))
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        assert pc.bits(loss) == pc.bits(eager) and torch.equal(grad, eg)
        assert stats.tolist() == cc.T("c_stats").tolist()
    panoptic.verify_major(block=True)                       # the captured calls' deferred verdicts


def test_panoptic_step_with_the_criterion_eager_and_captured(dev):
    """``SPTPanopticStep(criterion=...)`` on the reference's demo room - its own label histograms,
    a seeded InstanceData on its level-1 nodes (the fixture stores no ``obj``) - eager, then
    captured: the inherited ``capture()`` works for the panoptic model."""
    import test_hist_loss_gpu as hl
    from superpoint_transformer_amd import csr, hotpath, panoptic, predict
    from superpoint_transformer_amd.criterion import (EdgeAffinityCriterion, PanopticCriterion,
                                                       SemanticCriterion)
    g = hl.fixture(torch.device("cpu"))
    levels = hl.demo_levels()

    class Nag:
        num_clouds = 1

        def __init__(self, levels):
            self.levels = levels
            self.num_points = [lv["pos"].shape[0] for lv in levels]

        def __getitem__(self, i):
            return self.levels[i]

    nag = Nag([{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in lv.items()} for lv in levels])
    n1 = nag.num_points[1]
    ei = levels[1]["edge_index"]
    ne = int((ei[0] < ei[1]).sum())
    obj = pc.random_instance(n1, 3, hotpath.NUM_CLASSES, seed=5)
    affinity = torch.from_numpy(np.random.default_rng(6).choice([0.0, 1.0, 0.5, 0.3], ne)
                                .astype(np.float32))

    def make():
        return PanopticCriterion(SemanticCriterion(hotpath.NUM_CLASSES, "ce_kl", weight=g["weight"]),
                                 EdgeAffinityCriterion(weighted=True, case_weights=[0.5, 4, 1, 2],
                                                       pos_weight=2.5), edge_affinity_loss_lambda=10)
    targets = {"y_hist": [g["y1"], g["y2"]], "obj": obj, "obj_edge_affinity": affinity}
    step = hotpath.SPTPanopticStep(nag, dev, seed=3, criterion=make(), targets=targets)
    seen = []
    hook = step.criterion.register_forward_hook(
        lambda mod, inp, out: seen.append(([l.detach().cpu().double() for l in inp[0]],
                                           inp[2].detach().cpu().double())))
    loss = float(step.step().detach())
    hook.remove()
    node_obj, _, node_y = panoptic.major_objects(obj, hotpath.NUM_CLASSES)
    oei = ei[:, ei[0] < ei[1]].contiguous()
    cpu = make()(seen[0][0], targets["y_hist"], seen[0][1], affinity.double(), oei,
                 predict.void_mask(g["y1"]), node_obj, node_y)
    cpu = float(cpu[0])
    print(f"eager loss {loss:.9g}, CPU criterion on the same logits {cpu:.9g}")
    assert np.isfinite(loss) and abs(loss - cpu) <= 1e-6 * max(1.0, abs(cpu))
    tp, fp, tn, fn = step.edge_stats.compute()
    assert tp + fp + tn + fn == int((~(predict.void_mask(g["y1"])[oei[0]]
                                       & predict.void_mask(g["y1"])[oei[1]])).sum())
    step.capture(warmup=1)
    assert step.graph is not None
    captured = float(step.step().detach())
    torch.cuda.synchronize()
    csr.verify_adopted(block=True)
    print(f"captured loss {captured:.9g}")
    assert np.isfinite(captured)


def test_panoptic_step_without_a_criterion_is_the_stand_in(dev):
    """No criterion: the step of before - plain CE on its seeded labels plus BCE on its seeded
    0 / 1 affinities - now through the inherited ``step()``; it captures too."""
    import test_hist_loss_gpu as hl
    from superpoint_transformer_amd import csr, hotpath
    levels = hl.demo_levels()

    class Nag:
        num_clouds = 1

        def __init__(self, levels):
            self.levels = levels
            self.num_points = [lv["pos"].shape[0] for lv in levels]

        def __getitem__(self, i):
            return self.levels[i]

    nag = Nag([{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in lv.items()} for lv in levels])
    step = hotpath.SPTPanopticStep(nag, dev, seed=3)
    assert step.criterion is None and step.targets is None
    seen = []
    # (detached: an output kept with its grad_fn would keep the eager step's autograd graph alive,
    # which capture() must not find - see its comment on AccumulateGrad nodes)
    hook = step.model.register_forward_hook(
        lambda mod, inp, out: seen.append(([l.detach() for l in out[0]], out[1].detach())))
    loss = float(step.step().detach())                       # (no reference to the eager graph)
    hook.remove()
    logits, aff = seen[0]
    want = sum(l * torch.nn.functional.cross_entropy(lg.double(), y)
               for l, lg, y in zip(step.lambdas, logits, step.labels))
    want = want + torch.nn.functional.binary_cross_entropy_with_logits(aff.double(),
                                                                        step.affinity.double())
    assert abs(loss - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    step.capture(warmup=1)
    assert np.isfinite(float(step.step().detach()))
    csr.verify_adopted(block=True)
