"""The comparisons of the partition criterion (``ops.partition_edge_loss``,
``criterion.PartitionCriterion``) against tests/golden/partition_criterion.npz - the reference's
own ``PartitionCriterion`` in eval mode, written by tests/golden/make_golden_partition_criterion.py
- and against the float64 host twin tests/partition_criterion_reference.py, shared by the CPU
route's tests and the device's: every function takes the device to run on.

Integers (labels, classes, counters, the selected mask) compare exactly.  Losses and gradients
fall under ``panoptic_cases.within``: the yardstick is the fixture's float64 evaluation, the bar
per element 4 x the reference's own f32 deviation from it and never below one f32 ulp of the value.
The measured deviations are in profiles/r25a_partition_criterion_errors.txt."""
import functools
import itertools

import numpy as np
import torch

import panoptic_cases as pc
import partition_criterion_reference as R
from conftest import load_golden

GAMMAS, WEIGHTS, TEMPERATURES = (0, 1, 2), (0.5, 0.8), (1, 0.25)
SETTINGS = list(itertools.product(GAMMAS, WEIGHTS, TEMPERATURES))
RATIOS = (0.9, 0.5, 0.1)


def tag(gamma, weight, temperature):
    return f"g{gamma}_w{int(weight * 10)}_t{int(temperature * 100)}"


@functools.lru_cache(maxsize=None)
def golden():
    g = load_golden("partition_criterion.npz")
    g.update(load_golden("partition_criterion_f64.npz"))
    return g


def T(key, dev="cpu"):
    return torch.from_numpy(np.asarray(golden()[key])).to(dev)


def scene(dev):
    return T("x", dev), T("y", dev), T("edge_index", dev), int(golden()["num_classes"])


@functools.lru_cache(maxsize=None)
def twin(gamma, weight, temperature, ratio=None, state=(0, 0)):
    """The twin on the fixture's scene, computed once per setting and shared."""
    g = golden()
    out = R.loss_and_grad(g["x"], g["y"], g["edge_index"], int(g["num_classes"]), temperature, gamma,
                          weight, 1e-6, ratio, state)
    out["grad"].setflags(write=False)
    out["selected"].setflags(write=False)
    return out


def run(dev, x, y, ei, c, gamma=0, weight=0.5, temperature=1, ratio=None, state=None, grad=True):
    """One call on fresh buffers: loss, gradient, counts, status, selected (host copies)."""
    from superpoint_transformer_amd import ops
    x = x.clone().requires_grad_(grad)
    counts = torch.full((3,), -7, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    selected = torch.full((ei.shape[1],), 9, dtype=torch.uint8, device=dev)
    loss = ops.partition_edge_loss(x, y, ei, c, temperature=temperature, gamma=gamma, weight=weight,
                                   ratio=ratio, state=state, counts=counts, status=status,
                                   selected=selected)
    g = torch.autograd.grad(loss, x)[0] if grad else None
    return loss.detach(), g, counts.cpu(), status.cpu(), selected.cpu()


def random_case(n, d, e, seed, c=5, spread=0.3):
    """numpy ``(x f32 [n, d], y int64 [n, c + 1], edge_index int64 [2, e])``: labels in runs of
    7 nodes, a void node every 11th (from node 5 on), edges between near nodes, a few far ones."""
    rng = np.random.default_rng(seed)
    block = (np.arange(n) // 7) % c
    y = np.zeros((n, c + 1), dtype=np.int64)
    y[np.arange(n), block] = rng.integers(1, 9, n)
    y[:, c] = rng.integers(0, 3, n)
    y[5::11, :c] = 0
    i = rng.integers(0, n, e)
    j = (i + rng.integers(-4, 5, e)) % n            # (offset 0: a self loop now and then)
    far = rng.random(e) < 0.1
    j = np.where(far, rng.integers(0, n, e), j)
    x = (rng.normal(size=(n, d)) * spread + block[:, None] * 0.2).astype(np.float32)
    return x, y, np.stack([i, j]).astype(np.int64)


def check_against_twin(dev, x, y, ei, c, gamma=2, weight=0.8, temperature=0.5, ratio=None,
                       state=None, bad=0):
    """One call on ``dev`` against the twin on the same arrays: decisions exact; the loss and
    every element of the gradient within one f32 ulp of the twin's float64 value (the package
    rounds a float64 sum to f32 once: half an ulp) plus 2^-45 of the largest gradient entry (the
    two float64 sums run in different orders).  Returns the call's results."""
    want = R.loss_and_grad(x, y, ei, c, temperature, gamma, weight, 1e-6, ratio,
                           tuple(state) if state is not None else (0, 0))
    st = torch.tensor(list(state), dtype=torch.int64, device=dev) if state is not None else None
    got = run(dev, *(torch.from_numpy(a).to(dev) for a in (x, y, ei)), c, gamma, weight, temperature,
              ratio, st)
    loss, grad, counts, status, selected = got
    assert counts.tolist() == list(want["counts"])
    assert np.array_equal(selected.numpy().astype(bool), want["selected"])
    assert status.tolist() == [bad, want["clamped"]] and want["bad"] == bad
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert abs(float(loss) - want["loss"]) <= float(np.spacing(np.float32(abs(want["loss"]))))
    bar = np.spacing(np.abs(want["grad"]).astype(np.float32)).astype(np.float64) \
        + 2.0 ** -45 * np.abs(want["grad"]).max()
    err = np.abs(grad.cpu().double().numpy() - want["grad"])
    assert (err <= bar).all(), (err.max(), np.abs(want["grad"]).max())
    return got, want


# ---- the twin against the reference --------------------------------------------------------------
def check_twin_against_fixture():
    g = golden()
    code, bad = R.classify(g["y"], g["edge_index"], int(g["num_classes"]))
    assert bad == 0
    assert np.array_equal(R.node_labels(g["y"], int(g["num_classes"])), g["label"])
    assert np.array_equal(code != 0, g["keep"]) and np.array_equal(code == 2, g["intra"])
    assert R.major_count(int(g["n_inter"]), float(g["ratio"])) == int(g["n_major"])
    report = {}
    for s in SETTINGS:
        t, key = twin(*s), tag(*s)
        assert t["counts"] == (int(g["n_inter"]), int(g["n_intra"]), int(g["keep"].sum()))
        # float64 against float64: the order of the sums differs - and the class weights: the
        # reference forms them as `y.float() * weight + (1 - y.float()) * (1 - weight)`, in f32
        # whatever the precision of p, so its weights are the f32 roundings of weight and
        # 1 - weight (relative error up to 2^-24 each, none for 0.5); here they stay float64
        rel = 1e-13 if float(np.float32(s[1])) == s[1] else 2.0 ** -24
        assert abs(t["loss"] - float(g[f"f64__{key}_loss"])) <= rel * abs(t["loss"]), key
        scale = np.abs(g[f"f64__{key}_grad"]).max()
        assert np.abs(t["grad"] - g[f"f64__{key}_grad"]).max() <= 10 * rel * scale, key
        report[key] = (abs(t["loss"] - float(g[f"f64__{key}_loss"])),
                       np.abs(t["grad"] - g[f"f64__{key}_grad"]).max())
    return report


# ---- the package against the reference and the twin ----------------------------------------------
def check_fixture(dev):
    """Every setting of the fixture; returns {name: (our deviation, the reference's)}."""
    g = golden()
    x, y, ei, c = scene(dev)
    report = {}
    for s in SETTINGS:
        key = tag(*s)
        loss, grad, counts, status, selected = run(dev, x, y, ei, c, *s)
        assert loss.dtype == torch.float32 and grad.dtype == torch.float32
        assert counts.tolist() == list(twin(*s)["counts"]), key
        assert counts[0] == int(g["n_inter"]) and counts[1] == int(g["n_intra"])
        assert status.tolist() == [0, 0]
        assert np.array_equal(selected.numpy().astype(bool), g["keep"]), key
        report[f"{key} loss"] = pc.within(loss, g[f"f32__{key}_loss"], g[f"f64__{key}_loss"],
                                          f"{key} loss")
        report[f"{key} grad"] = pc.within(grad, g[f"f32__{key}_grad"], g[f"f64__{key}_grad"],
                                          f"{key} grad")
        # and against the twin, with the same bar
        pc.within(grad, g[f"f32__{key}_grad"], twin(*s)["grad"], f"{key} grad against the twin")
        assert bool(torch.isfinite(grad).all())
    return report


def check_fake_losses(dev):
    """Every node void / one label only: loss exactly 0, an all-zero gradient, the counters."""
    g = golden()
    x, _, ei, c = scene(dev)
    for name in ("allvoid", "onelabel"):
        y = T(f"{name}_y", dev)
        for ratio in (None, 0.9):
            state = torch.zeros(2, dtype=torch.int64, device=dev) if ratio else None
            loss, grad, counts, status, selected = run(dev, x, y, ei, c, 1, 0.5, 1, ratio, state)
            assert pc.bits(loss) == pc.bits(torch.zeros((), dtype=torch.float32)), name
            assert float(loss) == float(g[f"{name}_loss"])
            assert not bool(grad.any()) and bool(torch.isfinite(grad).all()), name
            assert counts[0] == int(g[f"{name}_n_inter"]) == 0
            want = R.loss_and_grad(g["x"], g[f"{name}_y"], g["edge_index"], c, ratio=ratio)
            assert counts.tolist() == list(want["counts"]), (name, ratio)
            assert np.array_equal(selected.numpy().astype(bool), want["selected"])


def check_label_vector(dev):
    """A 1-D label vector with C for void decides like the histograms it stands for."""
    g = golden()
    x, y, ei, c = scene(dev)
    labels = torch.from_numpy(np.where(g["label"] < 0, c, g["label"])).to(dev)
    a = run(dev, x, y, ei, c, 1, 0.8, 0.25)
    for lab in (labels, labels.int()):
        b = run(dev, x, lab, ei, c, 1, 0.8, 0.25)
        assert pc.bits(a[0]) == pc.bits(b[0]) and pc.bits(a[1]) == pc.bits(b[1])
        assert a[2].tolist() == b[2].tolist()


def check_sampling(dev, ratio):
    """The selected mask, the counters and the clamp bit equal the twin's; the same state draws
    the same sample, an advanced one another; the loss is the twin's over that sample."""
    g = golden()
    x, y, ei, c = scene(dev)
    state = torch.tensor([1234, 5], dtype=torch.int64, device=dev)
    loss, grad, counts, status, selected = run(dev, x, y, ei, c, 2, 0.5, 1, ratio, state)
    want = twin(2, 0.5, 1, ratio, (1234, 5))
    assert state.tolist() == [1234, 6]                               # the call advanced the counter
    assert counts.tolist() == list(want["counts"])
    assert np.array_equal(selected.numpy().astype(bool), want["selected"])
    assert int(selected.sum()) == counts[2]
    assert status.tolist() == [0, want["clamped"]]
    n_inter, n_intra = int(g["n_inter"]), int(g["n_intra"])
    assert want["clamped"] == int(R.major_count(n_inter, ratio) > n_intra)
    if ratio == 0.1:
        assert 9 * n_inter > n_intra and want["clamped"] == 1        # what this ratio is here for
    ulp = float(np.spacing(np.float32(abs(want["loss"]))))
    assert abs(float(loss) - want["loss"]) <= ulp
    gulp = np.spacing(np.abs(want["grad"]).astype(np.float32)).astype(np.float64)
    assert (np.abs(grad.cpu().double().numpy() - want["grad"]) <= gulp).all()
    # the same state again: the same draw, bit for bit
    again = torch.tensor([1234, 5], dtype=torch.int64, device=dev)
    l2, g2, c2, _, s2 = run(dev, x, y, ei, c, 2, 0.5, 1, ratio, again)
    assert pc.bits(l2) == pc.bits(loss) and pc.bits(g2) == pc.bits(grad) and torch.equal(s2, selected)
    # the advanced state: another sample of the same size (unless every intra edge is taken)
    l3, _, c3, _, s3 = run(dev, x, y, ei, c, 2, 0.5, 1, ratio, state)
    assert state.tolist() == [1234, 7] and c3.tolist() == counts.tolist()
    want3 = twin(2, 0.5, 1, ratio, (1234, 6))
    assert np.array_equal(s3.numpy().astype(bool), want3["selected"])
    if not want["clamped"]:
        assert not torch.equal(s3, selected)


def check_criterion(dev):
    """``PartitionCriterion`` on a ``PartitionOutput``: eval mode does not sample, training mode
    does; ``n_inter_edge`` is a device tensor; another loss function is refused."""
    import pytest
    from superpoint_transformer_amd.criterion import BinaryFocalLoss, PartitionCriterion
    from superpoint_transformer_amd.output import PartitionOutput
    g = golden()
    x, y, ei, c = scene(dev)
    crit = PartitionCriterion(BinaryFocalLoss(gamma=2, weight=0.8), affinity_temperature=0.25,
                              adaptive_sampling_ratio=0.9, num_classes=c, sharding=4096, seed=77).to(dev)
    direct = run(dev, x, y, ei, c, 2, 0.8, 0.25)
    crit.eval()
    out = PartitionOutput(y, x.clone().requires_grad_(), ei)
    assert out.has_target
    loss, same = crit(out)
    assert same is out and pc.bits(loss) == pc.bits(direct[0])
    assert torch.is_tensor(out.n_inter_edge) and out.n_inter_edge.dim() == 0
    assert out.n_inter_edge.device.type == torch.device(dev).type and int(out.n_inter_edge) == int(g["n_inter"])
    assert pc.bits(torch.autograd.grad(loss, out.x)[0]) == pc.bits(direct[1])
    assert crit.state.tolist() == [77, 0]
    crit.train()
    sel = torch.zeros(ei.shape[1], dtype=torch.uint8, device=dev)
    loss, _ = crit(PartitionOutput(y, x.clone().requires_grad_(), ei), selected=sel)
    want = twin(2, 0.8, 0.25, 0.9, (77, 0))
    assert crit.state.tolist() == [77, 1] and crit.counts.tolist() == list(want["counts"])
    assert np.array_equal(sel.cpu().numpy().astype(bool), want["selected"])
    with pytest.raises(ValueError, match="BinaryFocalLoss"):
        PartitionCriterion(torch.nn.CrossEntropyLoss(), num_classes=c)
    with pytest.raises(ValueError, match="labels"):
        crit(PartitionOutput(None, x, ei))
    # the holder's own formula, stand-alone: the reference's focal loss of the kept edges
    t = twin(2, 0.8, 0.25)
    e, d, l, _ = R.edge_terms(g["x"], g["edge_index"], t["selected"], t["code"], 0.25, 2, 0.8, 1e-6)
    p = torch.from_numpy(np.exp(-d / 0.25))
    alone = BinaryFocalLoss(gamma=2, weight=0.8)(p, torch.from_numpy(t["code"][e] == 2))
    assert abs(float(alone) - t["loss"]) <= 1e-6 * abs(t["loss"])


def check_arguments(dev):
    """Refusals come before any launch (nothing below reaches a kernel)."""
    import pytest
    from superpoint_transformer_amd import ops
    x, y, ei, c = scene(dev)
    f = ops.partition_edge_loss
    with pytest.raises(ValueError, match="No edges found in batch."):
        f(x, y, ei[:, :0], c)
    with pytest.raises(ValueError, match="1 to 128"):
        f(torch.zeros(300, 129, device=dev), y, ei, c)
    with pytest.raises(ValueError, match=r"\[N, D\]"):
        f(x[0], y, ei, c)
    with pytest.raises(ValueError, match="histogram"):
        f(x, y[:, :5], ei, c)
    with pytest.raises(ValueError, match="histogram"):
        f(x, y.float(), ei, c)
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        f(x, y, ei.t(), c)
    with pytest.raises(ValueError, match="ratio"):
        f(x, y, ei, c, ratio=0.0)
    with pytest.raises(ValueError, match="ratio"):
        f(x, y, ei, c, ratio=1.5)
    with pytest.raises(ValueError, match="temperature"):
        f(x, y, ei, c, temperature=0)
    with pytest.raises(ValueError, match="epsilon"):
        f(x, y, ei, c, epsilon=0.5)
    with pytest.raises(ValueError, match="state"):
        f(x, y, ei, c, ratio=0.5, state=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="counts"):
        f(x, y, ei, c, counts=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="status"):
        f(x, y, ei, c, status=torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="selected"):
        f(x, y, ei, c, selected=torch.zeros(3, dtype=torch.uint8, device=dev))
    if torch.device(dev).type != "cpu":
        with pytest.raises(ValueError, match="lives on"):
            f(x, y.cpu(), ei, c)
