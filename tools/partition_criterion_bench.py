"""The partition criterion at train-batch size: ``ops.partition_edge_loss`` (csrc/partition_loss.hip)
forward and forward + backward against the reference's composition
(``PartitionCriterion.edge_classification_loss`` + ``BinaryFocalLoss``,
src/loss/partition_criterion.py:92-145, src/loss/focal.py:194-220) restated in torch on the same
device and the same inputs.  The yardstick is that composition, never the new code itself.

The batch: ``--n`` voxels (default 1.2 M) on distinct cells of a 0.1 m lattice, 100 m x 100 m x 4
layers; the directed k = 8 kNN graph of ``transforms.KNN`` -> ``AdjacencyGraph`` (about 8 N edges);
labels constant on 5 m cells (13 classes), every 50th voxel void; D = 32 features.

Legs, each at ``ratio`` None (evaluation: every kept edge) and 0.9 (training: the adaptive sample):
  forward; forward + backward (the edge views of the fixed graph memoised, as in a training run);
  the two CSR builds of the edge views on their own; host reads and kernel launches of one call;
  peak memory above the inputs.  ``--step``: ``hotpath.SPTPartitionStep`` on the same batch, eager
  against captured, ms per step.

    python tools/partition_criterion_bench.py [--n N] [--reps R] [--step] [--rehearse]

``--rehearse``: the new legs once on CPU tensors at a small size, nothing timed (no GPU needed).
Per leg: device-time median and minimum over ``--reps`` calls after two warm-up calls and a
settle pause, host wall median.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from predict_bench import host_reads, launches, timed  # noqa: E402
from superpoint_transformer_amd import csr, ops  # noqa: E402

C, D, K = 13, 32, 8
GAMMA, WEIGHT, EPS, TEMPERATURE = 1.0, 0.5, 1e-6, 1.0          # default_ezsp.yaml


def batch(n, dev, rehearse=False):
    gen = torch.Generator(device=dev).manual_seed(25)
    side = max(int((n / 1.2) ** 0.5), 8)                        # 30 % of the cells of 4 layers
    cells = torch.randperm(side * side * 4, generator=gen, device=dev)[:n]
    coords = torch.stack((cells // (4 * side), (cells // 4) % side, cells % 4), dim=1)
    pos = coords.float() * 0.1
    block = (coords[:, 0] // 50) * 7 + (coords[:, 1] // 50) * 3
    label = block % C
    y = torch.zeros((n, C + 1), dtype=torch.int64, device=dev)
    y[torch.arange(n, device=dev), label] = torch.randint(1, 9, (n,), generator=gen, device=dev)
    y[::50, :C] = 0
    y[::50, C] = 1
    x = torch.randn((n, D), generator=gen, device=dev) * 0.2 + label[:, None] * 0.05
    if rehearse:                                                # no search kernels on the CPU
        nn = (torch.arange(n)[:, None] + torch.arange(1, K + 1)[None]) % n
        ei = torch.stack((torch.arange(n).repeat_interleave(K), nn.flatten()))
    else:
        from superpoint_transformer_amd import transforms as T
        from superpoint_transformer_amd.data import Data
        d = T.AdjacencyGraph(k=K, w=0.0)(T.KNN(k=K, r_max=0.5)(Data(pos=pos)))
        ei = d.edge_index.contiguous()
    return pos, coords, x, y, ei


def torch_loss(x, y, edge_index, ratio, backward):
    """The reference's steps, line by line, on device tensors."""
    x = x.detach().requires_grad_(backward)
    count, lab = y[:, :C].max(dim=1)
    edge_index = edge_index[:, ~(edge_index[0] == edge_index[1])]
    void = count == 0
    edge_index = edge_index[:, ~(void[edge_index[0]] | void[edge_index[1]])]
    if edge_index.numel() == 0:
        return None
    target = (lab[edge_index[0]] == lab[edge_index[1]]).int()
    n_inter = (target == 0).sum().item()
    if n_inter == 0:
        return None
    if ratio is not None:
        small = (target == 0).int().sum()
        large = target.shape[0] - small
        minority = torch.where(target == 0)[0]
        n_major = ((1 / ratio - 1) * small).int()
        assert n_major <= large
        majority = torch.where(target != 0)[0]
        majority = majority[torch.randperm(large, device=target.device)[:n_major]]
        idx = torch.cat((minority, majority))
        edge_index, target = edge_index[:, idx], target[idx]
    d = torch.norm(x[edge_index[0]] - x[edge_index[1]], dim=-1, p=2)
    p = torch.exp(-d / TEMPERATURE)
    t = target.bool()
    p = (~t).float() + p * (2 * t.float() - 1)
    p = EPS + (1 - 2 * EPS) * p
    w = t.float() * WEIGHT + (1 - t.float()) * (1 - WEIGHT)
    loss = (-(1 - p) ** GAMMA * torch.log(p) * w).mean()
    if backward:
        loss.backward()
    return loss.detach(), x.grad, n_inter


def new_loss(x, y, ei, ratio, backward, state, counts):
    x = x.detach().requires_grad_(backward)
    loss = ops.partition_edge_loss(x, y, ei, C, TEMPERATURE, GAMMA, WEIGHT, EPS, ratio=ratio,
                                   state=state, counts=counts)
    if backward:
        loss.backward()
    return loss.detach(), x.grad


def peak_mib(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_200_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        dev, a.n = torch.device("cpu"), min(a.n, 20_000)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: timings are taken on the MI355X only (--rehearse runs the new "
                             "legs once on the CPU)")
        dev = torch.device("cuda:0")
    pos, coords, x, y, ei = batch(a.n, dev, a.rehearse)
    state = torch.tensor([25, 0], dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    for ratio in (None, 0.9):
        loss, grad = new_loss(x, y, ei, ratio, True, state, counts)
        print(f"n {a.n}, edges {ei.shape[1]}, D {D}, ratio {ratio}: loss {float(loss):.7f}, n_inter / "
              f"n_intra / n_selected {counts.tolist()}, |grad| max {float(grad.abs().max()):.3e}")
    if a.rehearse:
        return
    ref = torch_loss(x, y, ei, None, True)
    loss, grad = new_loss(x, y, ei, None, True, state, counts)
    scale = float(ref[1].abs().max())
    print(f"ratio None: loss {float(loss):.7f} against the restatement's {float(ref[0]):.7f} (f32 there); "
          f"largest gradient difference / largest gradient "
          f"{float((grad - ref[1]).abs().max()) / scale:.2e}; n_inter equal: {ref[2] == int(counts[0])}")

    def views():
        csr.forget(ei)
        return csr.edge_end_views(ei, a.n)

    print(f"{'leg':<58}{'ms median':>11}{'ms min':>9}{'wall ms':>9}{'launches':>10}{'host reads':>12}"
          f"{'peak MiB':>10}")
    table = []
    for ratio in (None, 0.9):
        for backward in (False, True):
            what = "fwd + bwd" if backward else "fwd"
            table.append((f"new, {what}, ratio {ratio}",
                          lambda r=ratio, b=backward: new_loss(x, y, ei, r, b, state, counts)))
            table.append((f"torch, {what}, ratio {ratio}",
                          lambda r=ratio, b=backward: torch_loss(x, y, ei, r, b)))
    table.append(("new, the two CSR builds of the edge views alone", views))
    for name, fn in table:
        med, best, wall = timed(fn, a.reps)
        print(f"{name:<58}{med:>11.3f}{best:>9.3f}{wall:>9.2f}{launches(fn):>10}{host_reads(fn):>12}"
              f"{peak_mib(fn, dev):>10.1f}")
    if a.step:
        step_legs(pos, coords, x, y, ei, dev, a.reps)


def step_legs(pos, coords, x, y, ei, dev, reps):
    from superpoint_transformer_amd.criterion import BinaryFocalLoss, PartitionCriterion
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.hotpath import SPTPartitionStep

    def make():
        crit = PartitionCriterion(BinaryFocalLoss(gamma=GAMMA), TEMPERATURE, 0.9, C, None, seed=25)
        d = Data(pos=pos, coords=coords, x=x[:, :7].contiguous(), y=y, edge_index=ei)
        return SPTPartitionStep(d, dev, crit, cnn=[7, 32, 32, 32])

    eager = make()
    med, best, wall = timed(lambda: eager.step(), reps)
    print(f"{'SPTPartitionStep eager, ms per step':<58}{med:>11.3f}{best:>9.3f}{wall:>9.2f}"
          f"{launches(lambda: eager.step()):>10}{host_reads(lambda: eager.step()):>12}")
    del eager
    path = make().capture(warmup=2)
    med, best, wall = timed(lambda: path.step(), reps)
    print(f"{'SPTPartitionStep captured, ms per step':<58}{med:>11.3f}{best:>9.3f}{wall:>9.2f}"
          f"{'1 graph':>10}{host_reads(lambda: path.step()):>12}")


if __name__ == "__main__":
    main()
