"""CPU suite of the default semantic criterion and the histogram confusion matrix
(superpoint_transformer_amd.criterion / .metrics on the sync-free torch composition of
ops.histogram_loss): the fixture tests/golden/criterion.npz holds what the reference's own
``loss_with_target_histogram`` and ``CrossEntropyLoss(weight, ignore_index)`` give in float64 on
the demo room's label histograms (tests/golden/make_golden_criterion.py).

Bars (those of tests/test_loss_gpu.py): loss within 1e-6 relative, d logits within 1e-6 of the
largest gradient entry.  The reference's ConfusionMatrix needs torchmetrics and torch_scatter,
which are not available: the confusion matrices are compared, with ``torch.equal``, with the
exact integer formula ``confmat[t, p] = sum_{r: pred_r = p} h[r, t]`` (the reference sums the same
counts in float32, exact while every cell stays below 2^24)."""
import pytest
import torch

from conftest import load_golden


def fixture():
    g = {k: torch.from_numpy(v) for k, v in load_golden("criterion.npz").items()}
    for k in ("y1", "y2", "y1v"):
        g[k] = g[k].long()
    return g


def close(a, b):
    return abs(float(a) - float(b)) <= 1e-6 * max(1.0, abs(float(b)))


def grad_close(g, ref):
    return float((g.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-12


def exact_confmat(pred, h, C):
    """confmat[t, p] = sum of h[r, t] over the rows predicted p, in integers."""
    onehot = torch.nn.functional.one_hot(pred, C)                  # [rows, C]
    return h[:, :C].t() @ onehot


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_single_stage_losses_reproduce_the_reference(weighted, dtype):
    from superpoint_transformer_amd.criterion import SemanticCriterion
    g = fixture()
    C, tag = g["z1"].shape[1], "w" if weighted else "u"
    for kind in ("ce", "kl"):
        crit = SemanticCriterion(C, loss_type=kind, weight=g["weight"] if weighted else None)
        for case, z, y in (("l1", "z1", "y1"), ("l2", "z2", "y2"), ("l1v", "z1", "y1v")):
            loss = crit(g[z].to(dtype), g[y])
            assert close(loss, g[f"{tag}_single_{kind}_{case}"]), (kind, case)


@pytest.mark.parametrize("loss_type", ["ce", "kl", "ce_kl"])
def test_multi_stage_losses_and_gradients_reproduce_the_reference(loss_type):
    from superpoint_transformer_amd.criterion import SemanticCriterion
    g = fixture()
    C = g["z1"].shape[1]
    crit = SemanticCriterion(C, loss_type=loss_type, lambdas=g["lambdas"].tolist())
    crit.weight = g["weight"]                                   # set after construction (on_fit_start)
    for dtype in (torch.float64, torch.float32):
        a = [g["z1"].to(dtype).requires_grad_(), g["z2"].to(dtype).requires_grad_()]
        loss = crit(a, [g["y1v"], g["y2"]])
        assert close(loss.detach(), g[f"w_multi_{loss_type}"])
        g1, g2 = torch.autograd.grad(loss, a)
        assert grad_close(g1, g[f"w_multi_{loss_type}_g1"])
        assert grad_close(g2, g[f"w_multi_{loss_type}_g2"])
    crit.weight = None
    loss = crit([g["z1"].double(), g["z2"].double()], [g["y1v"], g["y2"]])
    assert close(loss, g[f"u_multi_{loss_type}"])


def test_weighted_index_cross_entropy_is_torchs():
    from superpoint_transformer_amd import ops
    g = fixture()
    z, C = g["z1"].double().requires_grad_(), g["z1"].shape[1]
    t = g["y1v"].argmax(dim=1)
    loss = ops.cross_entropy(z, t, ignore_index=C, weight=g["weight"])
    zr = g["z1"].double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(zr, t, weight=g["weight"].double(), ignore_index=C)
    assert close(loss.detach(), ref.detach())
    assert grad_close(torch.autograd.grad(loss, z)[0], torch.autograd.grad(ref, zr)[0])


def test_refused_and_malformed_inputs_raise():
    from superpoint_transformer_amd import ops
    from superpoint_transformer_amd.criterion import SemanticCriterion
    for lt in ("wce", "wce_kl"):
        with pytest.raises(ValueError, match="advanced-index assignment"):
            SemanticCriterion(13, loss_type=lt)
    with pytest.raises(ValueError):
        SemanticCriterion(13, loss_type="focal")
    z = torch.randn(10, 13)
    for ncols in (12, 15):
        h = torch.ones(10, ncols, dtype=torch.long)
        with pytest.raises(ValueError, match="columns"):
            SemanticCriterion(13, "kl")(z, h)
        with pytest.raises(ValueError, match="columns"):
            ops.histogram_loss(z, h, mode="dominant")
    with pytest.raises(ValueError, match="single-stage"):
        SemanticCriterion(13, "ce_kl")(z, torch.ones(10, 14, dtype=torch.long))
    with pytest.raises(ValueError):
        SemanticCriterion(13, "ce_kl")([z, z], [torch.ones(10, 14, dtype=torch.long)])
    with pytest.raises(ValueError, match="at least 13 columns"):
        ops.histogram_confusion_matrix(z, torch.ones(10, 12, dtype=torch.long), 13)


def test_poisoned_and_empty_batches_give_nan():
    from superpoint_transformer_amd import ops
    z = torch.randn(6, 4)
    h = torch.randint(0, 9, (6, 5))
    assert torch.isfinite(ops.histogram_loss(z, h))
    bad = h.clone()
    bad[2, 1] = -1
    assert torch.isnan(ops.histogram_loss(z, bad)) and torch.isnan(ops.histogram_loss(z, bad, mode="dominant"))
    void = torch.zeros_like(h)
    void[:, 4] = 3
    assert torch.isnan(ops.histogram_loss(z, void * 0))            # H == 0: the reference's 0 / 0
    assert torch.isnan(ops.histogram_loss(z, void, mode="dominant"))


def test_confusion_matrix_is_the_exact_integer_formula():
    from superpoint_transformer_amd.metrics import ConfusionMatrix
    g = fixture()
    C = g["z1"].shape[1]
    cm = ConfusionMatrix(C)
    expect = torch.zeros(C, C, dtype=torch.long)
    for z, y in ((g["z1"], g["y1v"]), (g["z2"], g["y2"]), (g["z1"], g["y1"][:, :C])):
        cm.update(z, y)                                             # logits: first maximum
        expect += exact_confmat(z.argmax(dim=1), y, C)
    assert cm.compute().dtype == torch.int64 and torch.equal(cm.compute(), expect)
    assert int(expect.max()) < 1 << 24                              # where the reference's f32 sum is exact too
    cm2 = ConfusionMatrix(C)
    cm2.update(g["z2"].argmax(dim=1), g["y2"])                      # int predictions
    assert torch.equal(cm2.confmat, exact_confmat(g["z2"].argmax(dim=1), g["y2"], C))
    # 1-D targets: labels outside [0, C) are void
    gen = torch.Generator().manual_seed(1)
    pred = torch.randint(0, C, (5000,), generator=gen)
    t = torch.randint(-2, C + 3, (5000,), generator=gen)
    cm3 = ConfusionMatrix(C)
    cm3.update(pred, t)
    cm3.update(pred, t[:, None])
    ok = (t >= 0) & (t < C)
    expect = torch.zeros(C * C, dtype=torch.long).index_add_(0, t[ok] * C + pred[ok], torch.ones(int(ok.sum()), dtype=torch.long))
    assert torch.equal(cm3.confmat, 2 * expect.view(C, C))
    cm3.reset()
    assert int(cm3.confmat.sum()) == 0
    # from_histogram: every column a class, every row predicted as its dominant label
    h = g["y2"][:, :C]
    assert torch.equal(ConfusionMatrix.from_histogram(h).confmat, exact_confmat(h.argmax(dim=1), h, C))


def test_fused_confusion_matrix_of_the_criterion():
    from superpoint_transformer_amd.criterion import SemanticCriterion
    from superpoint_transformer_amd.metrics import ConfusionMatrix
    g = fixture()
    C = g["z1"].shape[1]
    cm = ConfusionMatrix(C)
    crit = SemanticCriterion(C, weight=g["weight"])
    loss = crit([g["z1"].double(), g["z2"].double()], [g["y1v"], g["y2"]], confmat=cm.confmat)
    assert close(loss, g["w_multi_ce_kl"])
    assert torch.equal(cm.confmat, exact_confmat(g["z1"].argmax(dim=1), g["y1v"], C))


def test_metric_accessors_on_a_hand_computed_table():
    """3 classes, class 2 absent from predictions and ground truth:
        confmat = [[5, 1, 0], [2, 2, 0], [0, 0, 0]]    (rows: true, columns: predicted)
    IoU_0 = 5 / (5 + 1 + 2) = 0.625, IoU_1 = 2 / (2 + 2 + 1) = 0.4; OA = 7 / 10;
    per-class accuracy 5 / 6 and 2 / 4."""
    from superpoint_transformer_amd.metrics import ConfusionMatrix
    cm = ConfusionMatrix.from_confusion_matrix(torch.tensor([[5, 1, 0], [2, 2, 0], [0, 0, 0]]))
    iou, seen = cm.iou()
    assert seen.tolist() == [True, True, False]
    assert iou.tolist() == pytest.approx([62.5, 40.0, 1e-6], abs=1e-4)
    assert cm.oa() == pytest.approx(70.0) and cm.oa(as_percent=False) == pytest.approx(0.7)
    assert float(cm.miou()) == pytest.approx((62.5 + 40.0) / 2, abs=1e-4)
    # an absent class counts as the literal 1 of the reference (also in percent)
    assert float(cm.miou(missing_as_one=True)) == pytest.approx((62.5 + 40.0 + 1) / 3, abs=1e-4)
    assert float(cm.miou(missing_as_one=True, as_percent=False)) == pytest.approx((0.625 + 0.4 + 1) / 3, abs=1e-6)
    assert float(cm.macc()) == pytest.approx(100 * (5 / 6 + 2 / 4) / 2, abs=1e-4)
    m = cm.all_metrics()
    assert m.oa == pytest.approx(70.0) and float(m.miou) == pytest.approx(51.25, abs=1e-4)
    assert m.seen_class.tolist() == [True, True, False] and m.iou_per_class.shape == (3,)
    empty = ConfusionMatrix(3)
    assert empty.oa() == 0 and empty.miou() == 0 and empty.macc() == 0
