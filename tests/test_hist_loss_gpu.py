"""GPU parity of the histogram-loss and confusion-matrix kernels (csrc/loss.hip: the reference's
default criterion, loss_type 'ce_kl' with class weights on label histograms) against their
float64 closed forms in torch, and of ``criterion.SemanticCriterion`` / ``metrics.ConfusionMatrix``
against the reference's own results (tests/golden/criterion.npz).

Bars (those of tests/test_loss_gpu.py): loss within 1e-6 relative, d logits within 1e-6 of the
largest gradient entry, a second call bit-identical.  Confusion matrices: ``torch.equal`` with
the exact integer formula ``confmat[t, p] = sum_{r: pred_r = p} h[r, t]`` (the reference's own
class needs torchmetrics and torch_scatter, which are not available; it sums the same counts in
float32, exact while every cell stays below 2^24)."""
import numpy as np
import pytest
import torch

from conftest import demo_nag, load_golden, tl

pytestmark = pytest.mark.gpu

SHAPES = [(1, 13), (255, 13), (256, 13), (70_001, 13), (428_571, 13),
          (5000, 2), (5000, 16), (5000, 17), (5000, 19), (5000, 32)]


def make_case(rows, C, void, dev, seed=0):
    """Seeded logits, sparse label histograms and class weights.  From 8 rows up: row 0 is empty,
    row 1 all-void and row 2 void-dominant (with a void column), row 3 ties its first and last
    class (the first must win), and the logits of row 3 tie two maxima."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * C + int(void) + seed)
    ncols = C + int(void)
    z = torch.randn(rows, C, generator=g) * 3
    h = torch.randint(0, 60, (rows, ncols), generator=g) * (torch.rand(rows, ncols, generator=g) < 0.3)
    if rows >= 8:
        h[0] = 0
        if void:
            h[1] = 0
            h[1, C] = 11
            h[2, C] = h[2].max() + 1
        h[3] = 0
        h[3, 0] = h[3, C - 1] = 7
        z[3, 0] = z[3, C - 1] = z[3].max() + 1
    else:
        h[:, 0] += 1
        if void:
            h[:, C] = 0
    w = 0.4 + 1.6 * torch.rand(C, generator=g)
    return z.to(dev), h.to(dev), w.to(dev)


def closed_form(zd, h, w, mode):
    """float64 closed forms (ISSUE / DESIGN): histogram and dominant-label loss."""
    C = zd.shape[1]
    if mode == "histogram":
        lse = torch.logsumexp(zd, dim=1)
        return (h[:, :C].double() * w * (lse[:, None] - zd)).sum() / h.sum().double()
    return torch.nn.functional.cross_entropy(zd, h.argmax(dim=1), weight=w, ignore_index=C)


def check(loss, grad, ref, ref_grad):
    print(f"loss {float(loss):.9g} ref {float(ref):.9g} rel {abs(float(loss) - float(ref)) / max(1.0, abs(float(ref))):.3e}"
          f"  grad err / max {float((grad.double() - ref_grad).abs().max()) / float(ref_grad.abs().max()):.3e}")
    assert abs(float(loss) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))
    assert float((grad.double() - ref_grad).abs().max()) <= 1e-6 * float(ref_grad.abs().max()) + 1e-12


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("void", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", ["histogram", "dominant"])
def test_histogram_loss_matches_the_closed_form(rows, C, void, weighted, mode, dev):
    from superpoint_transformer_amd import ops
    z, h, w = make_case(rows, C, void, dev)
    if rows >= 8:
        assert int(h[3].argmax()) == 0                      # the tie: first index
    z.requires_grad_()
    s = torch.tensor(0.37, device=dev)
    loss = ops.histogram_loss(z, h, weight=w if weighted else None, mode=mode)
    (loss * s).backward()
    zd = z.detach().double().requires_grad_()
    ref = closed_form(zd, h, w.double() if weighted else torch.ones(C, device=dev, dtype=torch.float64), mode)
    (ref * s.double()).backward()
    check(loss.detach(), z.grad, ref.detach(), zd.grad)
    loss2 = ops.histogram_loss(z.detach(), h, weight=w if weighted else None, mode=mode)
    assert float(loss2) == float(loss)


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("ignore", [False, True])
def test_weighted_index_cross_entropy_matches_torch(rows, C, ignore, dev):
    from superpoint_transformer_amd import ops
    z, _, w = make_case(rows, C, False, dev)
    g = torch.Generator().manual_seed(rows + C)
    t = torch.randint(0, C + int(ignore), (rows,), generator=g).to(dev)
    ii = C if ignore else -100
    if ignore and bool((t == C).all()):
        t[0] = 0
    z.requires_grad_()
    s = torch.tensor(0.37, device=dev)
    loss = ops.cross_entropy(z, t, ignore_index=ii, weight=w)
    (loss * s).backward()
    zd = z.detach().double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(zd, t, weight=w.double(), ignore_index=ii)
    (ref * s.double()).backward()
    check(loss.detach(), z.grad, ref.detach(), zd.grad)
    assert float(ops.cross_entropy(z.detach(), t, ignore_index=ii, weight=w)) == float(loss)
    if rows >= 8:                                           # a label that is neither a class nor ignored
        t[5] = C + 3
        assert torch.isnan(ops.cross_entropy(z.detach(), t, ignore_index=ii, weight=w)).item()


def exact_confmat(pred, h, C):
    """confmat[t, p] = sum of h[r, t] over the rows predicted p, in int64 on the CPU."""
    return torch.zeros(C, C, dtype=torch.long).index_add_(1, pred.cpu(), h.cpu()[:, :C].t().contiguous())


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("void", [False, True])
def test_confusion_matrix_fused_and_stand_alone(rows, C, void, dev):
    from superpoint_transformer_amd import ops
    z, h, w = make_case(rows, C, void, dev)
    pred = z.cpu().argmax(dim=1)                            # CPU argmax: first maximum
    if rows >= 8:
        assert int(pred[3]) == 0
    expect = exact_confmat(pred, h, C)
    assert int(expect.max()) < 1 << 24
    for mode in ("histogram", "dominant"):
        buf = torch.zeros(C, C, dtype=torch.long, device=dev)
        with_cm = ops.histogram_loss(z, h, weight=w, mode=mode, confmat=buf)
        assert torch.equal(buf.cpu(), expect)
        assert float(with_cm) == float(ops.histogram_loss(z, h, weight=w, mode=mode))
        ops.histogram_loss(z, h, weight=w, mode=mode, confmat=buf)          # accumulates
        assert torch.equal(buf.cpu(), 2 * expect)
    assert torch.equal(ops.histogram_confusion_matrix(z, h, C).cpu(), expect)
    assert torch.equal(ops.histogram_confusion_matrix(pred.to(dev), h, C).cpu(), expect)
    # 1-D targets: labels outside [0, C) are void
    g = torch.Generator().manual_seed(rows)
    t = torch.randint(-2, C + 3, (rows,), generator=g)
    ok = (t >= 0) & (t < C)
    e1 = torch.zeros(C * C, dtype=torch.long).index_add_(
        0, t[ok] * C + pred[ok], torch.ones(int(ok.sum()), dtype=torch.long)).view(C, C)
    assert torch.equal(ops.histogram_confusion_matrix(pred.to(dev), t.to(dev), C).cpu(), e1)
    assert torch.equal(ops.histogram_confusion_matrix(pred.to(dev), t.to(dev)[:, None], C).cpu(), e1)


def test_confusion_matrix_accumulates_over_updates(dev):
    from superpoint_transformer_amd.metrics import ConfusionMatrix
    C = 13
    cm = ConfusionMatrix(C, device=dev)
    expect = torch.zeros(C, C, dtype=torch.long)
    for seed, rows in ((1, 70_001), (2, 5000), (3, 255)):
        z, h, _ = make_case(rows, C, True, dev, seed=seed)
        cm.update(z, h)
        expect += exact_confmat(z.cpu().argmax(dim=1), h, C)
    assert cm.confmat.is_cuda and torch.equal(cm.compute().cpu(), expect)
    cpu = ConfusionMatrix.from_confusion_matrix(expect)
    assert cm.oa() == cpu.oa() and float(cm.miou()) == pytest.approx(float(cpu.miou()), rel=1e-6)
    assert float(cm.macc()) == pytest.approx(float(cpu.macc()), rel=1e-6)
    cm.reset()
    assert int(cm.confmat.sum()) == 0


def test_poisoned_and_empty_batches(dev):
    """A negative count makes the loss NaN (never a silently wrong mean); a batch with nothing to
    average over gives NaN like the reference's 0 / 0: every row void-dominant in 'dominant' mode,
    every row empty in 'histogram' mode.  An all-void batch in 'histogram' mode is 0 / H = 0, as in
    the reference (the void column counts in the denominator only)."""
    from superpoint_transformer_amd import ops
    z, h, w = make_case(1000, 13, True, dev)
    assert torch.isfinite(ops.histogram_loss(z, h, weight=w)).item()
    bad = h.clone()
    bad[17, 4] = -1
    assert torch.isnan(ops.histogram_loss(z, bad, weight=w)).item()
    assert torch.isnan(ops.histogram_loss(z, bad, weight=w, mode="dominant")).item()
    void = torch.zeros_like(h)
    void[:, 13] = 5
    assert torch.isnan(ops.histogram_loss(z, void, weight=w, mode="dominant")).item()
    assert float(ops.histogram_loss(z, void, weight=w)) == 0.0
    assert torch.isnan(ops.histogram_loss(z, torch.zeros_like(h), weight=w)).item()
    for ncols in (12, 15):
        with pytest.raises(ValueError, match="columns"):
            ops.histogram_loss(z, torch.ones(1000, ncols, dtype=torch.long, device=dev))


def fixture(dev):
    g = {k: torch.from_numpy(v).to(dev) for k, v in load_golden("criterion.npz").items()}
    for k in ("y1", "y2", "y1v"):
        g[k] = g[k].long()
    return g


@pytest.mark.parametrize("loss_type", ["ce", "kl", "ce_kl"])
def test_criterion_reproduces_the_reference_fixture(loss_type, dev):
    from superpoint_transformer_amd.criterion import SemanticCriterion
    from superpoint_transformer_amd.metrics import ConfusionMatrix
    g = fixture(dev)
    C = g["z1"].shape[1]
    crit = SemanticCriterion(C, loss_type=loss_type, lambdas=g["lambdas"].tolist(), weight=g["weight"]).to(dev)
    a = [g["z1"].clone().requires_grad_(), g["z2"].clone().requires_grad_()]
    cm = ConfusionMatrix(C, device=dev)
    loss = crit(a, [g["y1v"], g["y2"]], confmat=cm.confmat)
    g1, g2 = torch.autograd.grad(loss, a)
    check(loss.detach(), g1, g[f"w_multi_{loss_type}"], g[f"w_multi_{loss_type}_g1"])
    check(loss.detach(), g2, g[f"w_multi_{loss_type}"], g[f"w_multi_{loss_type}_g2"])
    assert torch.equal(cm.confmat.cpu(), exact_confmat(g["z1"].cpu().argmax(dim=1), g["y1v"], C))
    crit.weight = None
    ref = g[f"u_multi_{loss_type}"]
    assert abs(float(crit(a, [g["y1v"], g["y2"]])) - float(ref)) <= 1e-6 * abs(float(ref))
    if loss_type != "ce_kl":
        for tag, w in (("w", g["weight"]), ("u", None)):
            crit.weight = w
            for case, z, y in (("l1", "z1", "y1"), ("l2", "z2", "y2"), ("l1v", "z1", "y1v")):
                ref = g[f"{tag}_single_{loss_type}_{case}"]
                assert abs(float(crit(g[z], g[y])) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))


def test_criterion_is_capturable_and_replays_the_eager_loss(dev):
    """'ce_kl' with class weights on two levels, loss + backward inside torch.cuda.graph: a host
    synchronisation inside a capture raises, so capturing at all is the property the reference's
    where / repeat_interleave composition cannot have.  Replays give the eager loss bit for bit."""
    from superpoint_transformer_amd.criterion import SemanticCriterion
    g = fixture(dev)
    C = g["z1"].shape[1]
    crit = SemanticCriterion(C, "ce_kl", weight=g["weight"]).to(dev)
    y = [g["y1v"], g["y2"]]
    # the eager result on leaves of its own: a leaf's gradient accumulator remembers the stream it
    # was created on, and autograd synchronises that stream with the backward's - for leaves first
    # used on the default stream that pulls the default stream into the capture (unjoined work).
    # The captured leaves are first used in the warm-up, on the capture's own stream.
    b = [g["z1"].clone().requires_grad_(), g["z2"].clone().requires_grad_()]
    eager = crit(b, y)
    eg = [x.clone() for x in torch.autograd.grad(eager, b)]
    eager = eager.detach().clone()
    del b
    a = [g["z1"].clone().requires_grad_(), g["z2"].clone().requires_grad_()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                  # warm-up: allocator, workspace
            torch.autograd.grad(crit(a, y), a)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        loss = crit(a, y)
        grads = torch.autograd.grad(loss, a)
    for _ in range(2):
        loss.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert float(loss) == float(eager)
        assert all(torch.equal(p, q) for p, q in zip(grads, eg))


def demo_levels():
    """Levels 0-2 of the reference's demo room as the model's input (as in tests/test_model_gpu.py:
    the stored 7-D edge features zero-padded to the 18-D RPE input)."""
    lv = demo_nag()
    levels = []
    for i in range(3):
        d = dict(pos=torch.from_numpy(lv[i]["pos"]).float(),
                 super_index=tl(lv[i]["super_index"]) if i < 2 else None, batch=None, x=None)
        if i == 0:
            feats = [torch.from_numpy(lv[0][k]).float() for k in
                     ("linearity", "planarity", "scattering", "verticality", "elevation")]
            d["x"] = torch.cat(feats + [torch.from_numpy(lv[0]["rgb"]).float() / 255], dim=1)
        else:
            ei = tl(lv[i]["edge_index"])
            loops = torch.arange(d["pos"].shape[0])
            full = torch.cat([ei, ei.flip(0), torch.stack([loops, loops])], dim=1)
            ea7 = torch.from_numpy(lv[i]["edge_attr"]).float()
            ea = torch.zeros(full.shape[1], 18)
            ea[:ea7.shape[0], :7] = ea7
            ea[ea7.shape[0]:2 * ea7.shape[0], :7] = -ea7
            d["edge_index"], d["edge_attr"] = full, ea
            sub = lv[i]["sub_pointers"].astype(np.int64)
            d["node_size"] = torch.from_numpy(sub[1:] - sub[:-1]) if i == 1 else None
        levels.append(d)
    levels[2]["node_size"] = torch.zeros(levels[2]["pos"].shape[0], dtype=torch.long).index_add_(
        0, levels[1]["super_index"], levels[1]["node_size"])
    return levels


def test_train_step_with_the_default_criterion_eager_and_captured(dev):
    from superpoint_transformer_amd import csr, hotpath
    from superpoint_transformer_amd.criterion import SemanticCriterion
    g = fixture(torch.device("cpu"))
    levels = demo_levels()

    class Nag:
        num_clouds = 1

        def __init__(self, levels):
            self.levels = levels
            self.num_points = [lv["pos"].shape[0] for lv in levels]

        def __getitem__(self, i):
            return self.levels[i]

    nag = Nag([{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in lv.items()} for lv in levels])
    crit = SemanticCriterion(hotpath.NUM_CLASSES, "ce_kl", weight=g["weight"])
    targets = [g["y1"], g["y2"]]                            # the room's own label histograms
    step = hotpath.SPTTrainStep(nag, dev, seed=3, criterion=crit, targets=targets)
    seen = []
    hook = step.criterion.register_forward_hook(
        lambda mod, inp, out: seen.append([l.detach().cpu().double() for l in inp[0]]))
    loss = float(step.step().detach())
    hook.remove()
    cpu = float(SemanticCriterion(hotpath.NUM_CLASSES, "ce_kl", weight=g["weight"])(seen[0], targets))
    print(f"eager loss {loss:.9g}, CPU criterion on the same logits {cpu:.9g}")
    assert np.isfinite(loss) and abs(loss - cpu) <= 1e-6 * max(1.0, abs(cpu))
    step.capture(warmup=1)
    assert step.graph is not None
    captured = float(step.step().detach())
    torch.cuda.synchronize()
    csr.verify_adopted(block=True)
    print(f"captured loss {captured:.9g}")
    assert np.isfinite(captured)
