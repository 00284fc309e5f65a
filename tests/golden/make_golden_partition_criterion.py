"""Golden fixture for the partition criterion, produced by the REFERENCE'S OWN code:

  * ``PartitionCriterion`` (src/loss/partition_criterion.py), ``BinaryFocalLoss``
    (src/loss/focal.py), ``compute_edge_distances_batch`` (src/utils/batch_utils.py) and
    ``PartitionOutput`` (src/utils/output_partition.py), each loaded by file path; ``src.utils`` is
    a stub module holding the two names partition_criterion.py imports from it.

Scene: N = 300 nodes, D = 32, C = 13, E = 3 * 256 + 17 edges of which 27 are self loops; every 17th
node is void (its class columns are 0); histograms of two labels, with planted ties (the lower
label wins) - a tie between the block's label and a lower / a higher one; most edges join nodes a
few positions apart (blocks of 24 nodes share a label), the rest are random; nodes 40 and 41 hold
the same row and are joined in both directions (distance 0: the gradient of that edge is 0); a
duplicated edge.

The criterion runs in ``eval()`` mode (no sampling: deterministic) for gamma in {0, 1, 2} x weight
in {0.5, 0.8} x temperature in {1, 0.25}, in f32 (``f32__*``) and in f64 (``f64__*``, the
yardstick): the loss, ``x.grad`` and ``n_inter_edge``.  Two more cases on the same graph: every
node void, and one label only - both return the reference's fake loss 0.

The f64 gradients go to a file of their own (``partition_criterion_f64.npz``): twelve [300, 32]
f64 arrays do not fit one committed file.

Usage (build container only): python tests/golden/make_golden_partition_criterion.py [--check]
(``--check``: regenerate and compare with the committed files array by array, bit for bit).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import grid_sampling_reference as R  # noqa: E402

NAME, NAME64 = "partition_criterion.npz", "partition_criterion_f64.npz"
N, D, C = 300, 32, 13
E, LOOPS = 3 * 256 + 17, 27
GAMMAS, WEIGHTS, TEMPERATURES = (0, 1, 2), (0.5, 0.8), (1, 0.25)
RATIO = 0.9                                   # the config's adaptive_sampling_ratio (not drawn here)


def tag(gamma, weight, temperature):
    return f"g{gamma}_w{int(weight * 10)}_t{int(temperature * 100)}"


def by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(mg.REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("src", "src.loss"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
    batch = by_path("_ref_batch_utils", "src", "utils", "batch_utils.py")
    outp = by_path("_ref_output_partition", "src", "utils", "output_partition.py")
    stub = types.ModuleType("src.utils")
    stub.PartitionOutput = outp.PartitionOutput
    stub.compute_edge_distances_batch = batch.compute_edge_distances_batch
    sys.modules["src.utils"] = stub
    focal = by_path("src.loss.focal", "src", "loss", "focal.py")
    crit = by_path("src.loss.partition_criterion", "src", "loss", "partition_criterion.py")
    return crit.PartitionCriterion, focal.BinaryFocalLoss, outp.PartitionOutput


def scene(rng):
    block = (np.arange(N) // 24) % C
    y = np.zeros((N, C + 1), dtype=np.int64)
    for n in range(N):
        a = int(block[n])
        b = int(rng.integers(0, C - 1))
        b += b >= a
        ca = int(rng.integers(5, 40))
        y[n, a] += ca
        y[n, b] += int(rng.integers(1, ca))           # the block's label keeps the majority
        y[n, C] = int(rng.integers(0, 6))
    for n in range(3, N, 29):                         # planted ties: the lower label wins
        a = int(block[n])
        b = (a + 1) % C if (n // 29) % 2 else (a - 1) % C
        y[n, :C] = 0
        y[n, a] = y[n, b] = 7
    y[::17, :C] = 0                                   # void nodes (their void column may be 0 too)
    y[::17, C] = rng.integers(0, 9, len(y[::17]))
    i = rng.integers(0, N, E)
    j = (i + rng.integers(1, 9, E) * rng.choice([-1, 1], E)) % N
    far = rng.permutation(E)[:120]
    j[far] = rng.integers(0, N, 120)
    loop = i == j
    j[loop] = (i[loop] + 1) % N
    ei = np.stack([i, j]).astype(np.int64)
    ei[:, 100] = (40, 41)                             # the two identical rows, both directions
    ei[:, 101] = (41, 40)
    ei[:, 300] = ei[:, 299]                           # a duplicated edge
    free = np.array([e for e in range(102, E) if e not in (299, 300)])
    pick = rng.permutation(free)[:LOOPS]
    ei[1, pick] = ei[0, pick]
    x = (rng.normal(size=(N, D)) * 0.12 + rng.normal(size=(C, D))[block] * 0.1).astype(np.float32)
    x[41] = x[40]
    return x, y, ei


def run(PC, BFL, PO, x, y, ei, dtype, gamma, weight, temperature):
    T = torch.from_numpy
    crit = PC(loss_function=BFL(gamma=gamma, weight=weight), affinity_temperature=temperature,
              adaptive_sampling_ratio=RATIO, num_classes=C, sharding=None).eval()
    xt = T(x).to(dtype).requires_grad_()
    loss, out = crit(PO(T(y), xt, T(ei)))
    if out.n_inter_edge == 0:                         # the fake loss: a fresh leaf, no graph to x
        return loss.detach().to(dtype), torch.zeros_like(xt), 0
    grad = torch.autograd.grad(loss, xt)[0]
    return loss.detach(), grad, out.n_inter_edge


def build():
    torch.set_num_threads(1)
    PC, BFL, PO = load_reference()
    rng = np.random.default_rng(20261021)
    x, y, ei = scene(rng)
    out = {"num_classes": np.int64(C), "x": x, "y": y, "edge_index": ei, "ratio": np.float64(RATIO)}
    out64 = {}
    # what the scene was built to hold (the reference's own rules, restated on the host)
    best = y[:, :C].max(1)
    label = y[:, :C].argmax(1)
    void = best == 0
    assert int(void.sum()) == len(range(0, N, 17))
    assert int((ei[0] == ei[1]).sum()) == LOOPS, int((ei[0] == ei[1]).sum())
    keep = (ei[0] != ei[1]) & ~void[ei[0]] & ~void[ei[1]]
    intra = keep & (label[ei[0]] == label[ei[1]])
    n_inter, n_intra = int((keep & ~intra).sum()), int(intra.sum())
    n_major = int((torch.tensor(n_inter).int() * (1 / RATIO - 1)).int())
    assert n_inter >= 100 and n_intra >= 200 and 0 < n_major <= n_intra, (n_inter, n_intra, n_major)
    ties = [n for n in range(N) if not void[n] and (y[n, :C] == best[n]).sum() > 1]
    assert len(ties) >= 8
    out.update(label=np.where(void, -1, label).astype(np.int64), keep=keep, intra=intra,
               n_inter=np.int64(n_inter), n_intra=np.int64(n_intra), n_major=np.int64(n_major))
    for gamma in GAMMAS:
        for weight in WEIGHTS:
            for temperature in TEMPERATURES:
                t = tag(gamma, weight, temperature)
                for dtype, pre, dst in ((torch.float32, "f32__", out), (torch.float64, "f64__", out64)):
                    loss, grad, ni = run(PC, BFL, PO, x, y, ei, dtype, gamma, weight, temperature)
                    assert ni == n_inter
                    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), t
                    out[f"{pre}{t}_loss"] = loss
                    dst[f"{pre}{t}_grad"] = grad
    # every node void / one label only: the fake loss
    y_void = y.copy()
    y_void[:, :C] = 0
    y_one = np.zeros_like(y)
    y_one[:, 4] = 3
    for name, yy in (("allvoid", y_void), ("onelabel", y_one)):
        loss, grad, ni = run(PC, BFL, PO, x, yy, ei, torch.float32, 1, 0.5, 1)
        assert float(loss) == 0.0 and ni == 0 and not bool(grad.any())
        out[f"{name}_y"] = yy
        out[f"{name}_loss"] = loss
        out[f"{name}_n_inter"] = np.int64(ni)
    return out, out64


def main():
    out, out64 = build()
    for name, arrays in ((NAME, out), (NAME64, out64)):
        path = os.path.join(HERE, name)
        if "--check" in sys.argv:
            old = dict(np.load(path))
            assert set(old) == set(arrays), sorted(set(old) ^ set(arrays))
            for k, v in arrays.items():
                v = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
                assert R.bits_equal(old[k], v), f"{k} differs from the committed fixture"
            print(f"{name}: {len(arrays)} arrays bit-identical to the regenerated ones")
            continue
        mg.save(name, **arrays)
        print(f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
