"""GPU suite of ``GridSampling3D`` (csrc/voxel.hip, voxel.py, transforms.GridSampling3D).

Fixture cases (tests/golden/grid_sampling.npz: output of the reference's own code): everything
integer or boolean is exact; a mean's deviation from the f64 restatement, max |diff| / max |f64|,
must stay within 4 x the reference's own deviation for that key (exactly equal where that is 0).
Figures measured on an MI355X, kernel / reference, worst case over the fixture's cases (also in
profiles/r16a_grid_sampling_errors.txt):
    pos 1.538e-08 / 1.538e-08, rgb 5.045e-07 / 5.045e-07, intensity 1.723e-07 / 1.723e-07,
    normal 1.075e-07 / 1.075e-07.  The means of pos, rgb and intensity equal the reference's bit
    for bit; normal differs from it in the last place after the division by its norm.

Generated clouds are checked against the restatement (tests/grid_sampling_reference.py).  Bounds:
  * groups, histograms, votes, representatives: exact;
  * means of voxels of at most 512 points: BIT-EQUAL to the restatement's f32 ``index_add_`` mean
    (the same sum in the same order, one correctly rounded division);
  * means of longer voxels (summed by a fixed 64-lane tree): |mean - f64 mean| <=
    (ceil(n / 64) + 6 + 1) * 2^-24 * mean |x| - the standard bound (Higham, Accuracy and Stability,
    eq. 4.4) of a sum whose longest chain has ceil(n / 64) + 6 additions, plus the division.
"""
import math

import numpy as np
import pytest
import torch

import grid_sampling_reference as R
from guarded import GuardedArena, exact_workspaces
from test_grid_sampling_reference_cpu import (assert_reproduces, expected, reference_deviation,
                                              run_package)

pytestmark = pytest.mark.gpu

LONG_RUN = 512            # csrc/voxel.hip: longer runs are summed by a wave
N_BINS = 14


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def ref_deviation(golden):
    return reference_deviation(golden)


# ---- fixture cases on the device ---------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_fixture_case_on_the_device(golden, ref_deviation, case, dev):
    kwargs, with_batch = R.CASES[case]
    fields = R.golden_fields(golden, with_batch)
    out, _ = run_package(fields, kwargs, device=dev)
    mean_mode = kwargs.get("mode", "mean") == "mean"
    float_keys = [k for k in R.MEAN_KEYS if mean_mode and f"{case}__{k}" in golden]
    exact = {k: v for k, v in out.items() if k not in float_keys}
    want = {k: v for k, v in expected(golden, case).items()
            if k[len(case) + 2:] not in float_keys}
    assert_reproduces(want, case, exact, "package on the device")      # ints, bools, last-mode rows
    if not float_keys:
        return
    m64 = R.grid_sampling(fields, dtype=torch.float64, **kwargs)
    for k in float_keys:
        got = out[k].numpy()
        assert got.dtype == np.float32 and got.shape == golden[f"{case}__{k}"].shape
        mine = R.relative_deviation(got, m64[k].numpy())
        theirs = ref_deviation[k]
        same = R.bits_equal(got, golden[f"{case}__{k}"])
        print(f"\n{case} {k}: kernel {mine:.3e}, reference {theirs:.3e} (worst case), "
              f"bit-equal to the reference: {same}")
        if theirs == 0:
            assert mine == 0
        assert mine <= 4 * theirs, f"{case} {k}: {mine:.3e} > 4 x {theirs:.3e}"


# ---- generated clouds --------------------------------------------------------------------------
def cloud(n, size, seed, per_voxel=3.0):
    g = torch.Generator().manual_seed(seed)
    extent = max((n / per_voxel) ** (1 / 3), 1.0) * size
    return (torch.rand(n, 3, generator=g) - 0.5) * extent


def labels_for(n, n_bins, seed):
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, n_bins, (n,), generator=g)
    y[0] = 0
    y[-1] = n_bins - 1 if n > 1 else 0
    return y


def check_groups(g, pos, size, batch=None):
    """The groups against the restatement, and their own invariants."""
    coords, cluster, perm = R.voxelize(pos, size, batch)
    v = perm.numel()
    assert g.num_voxels == v and g.num_points == pos.shape[0]
    assert torch.equal(g.cluster.cpu(), cluster)
    order = g.order.cpu()
    assert torch.equal(order, torch.sort(cluster, stable=True).indices)
    ptr = g.pointers.cpu()
    assert torch.equal(ptr[1:] - ptr[:-1], torch.bincount(cluster, minlength=v)) and int(ptr[0]) == 0
    # inside every voxel the order is ascending, and `last` is the voxel's highest index
    inner = torch.ones(order.numel(), dtype=torch.bool)
    inner[ptr[:-1]] = False
    assert bool((order[1:] > order[:-1])[inner[1:]].all())
    top = torch.zeros(v, dtype=torch.long).scatter_reduce_(0, cluster, torch.arange(cluster.numel()), "amax")
    assert torch.equal(g.last.cpu(), top) and torch.equal(top, perm)
    assert g.coords.dtype == torch.int32
    assert torch.equal(g.coords.cpu().float(), coords[perm])
    return cluster, v


def mean_bound(n):
    return (math.ceil(n / 64) + 6 + 1) * 2.0 ** -24


def check_mean(x_dev, x_cpu, g, cluster, v, normalize=False):
    from superpoint_transformer_amd import voxel
    got = voxel.group_mean(x_dev, g, normalize=normalize).cpu()
    want = R.scatter_mean(x_cpu, cluster, v)
    counts = torch.bincount(cluster, minlength=v)
    short = counts <= LONG_RUN
    if normalize:
        want = want / want.norm(dim=1).view(-1, 1)
        # (the norm's own rounding: 3 products, 2 sums, a root, a division - a few ulp)
        assert torch.allclose(got, want, rtol=8 * 2.0 ** -24, atol=0, equal_nan=True)
        return got
    assert got.shape == want.shape and got.dtype == torch.float32
    assert R.bits_equal(got[short].numpy(), want[short].numpy()), "a short voxel's mean is not bit-equal"
    if not bool(short.all()):
        x64 = x_cpu.double()
        m64 = R.scatter_mean(x64, cluster, v)
        mabs = R.scatter_mean(x64.abs(), cluster, v)
        for i in torch.where(~short)[0].tolist():
            err = (got[i].double() - m64[i]).abs()
            assert bool((err <= mean_bound(int(counts[i])) * mabs[i]).all()), (i, err, mabs[i])
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 100_003])
def test_generated_cloud_against_the_restatement(n, dev):
    from superpoint_transformer_amd import voxel
    size = 0.05
    pos = cloud(n, size, seed=n)
    # pos as a column block of a wider table: row stride 8, not 3
    table = torch.zeros(n, 8)
    table[:, 2:5] = pos
    table_dev = table.to(dev)
    pos_dev = table_dev[:, 2:5]
    assert pos_dev.stride(0) == 8
    g = voxel.voxel_groups(pos_dev, size)
    cluster, v = check_groups(g, pos, size)
    g2 = voxel.voxel_groups(pos.to(dev), size)                       # contiguous: the same groups
    for a, b in ((g.pointers, g2.pointers), (g.cluster, g2.cluster), (g.order, g2.order),
                 (g.last, g2.last), (g.coords, g2.coords)):
        assert torch.equal(a, b)                                     # and two calls are bitwise equal

    gen = torch.Generator().manual_seed(7 * n + 1)
    x7 = torch.randn(n, 7, generator=gen) * 3 + 10
    x7_dev = x7.to(dev)
    views = [(x7_dev, x7), (x7_dev[:, 0], x7[:, 0]), (x7_dev[:, :1], x7[:, :1]),
             (x7_dev[:, 2:5], x7[:, 2:5]), (x7_dev[:, 3].contiguous(), x7[:, 3].contiguous())]
    for xd, xc in views:
        a = check_mean(xd, xc, g, cluster, v)
        assert torch.equal(a, voxel.group_mean(xd, g).cpu())         # bitwise reproducible
    check_mean(x7_dev[:, 2:5], x7[:, 2:5], g, cluster, v, normalize=True)

    y = labels_for(n, N_BINS, n)
    y_dev = y.to(dev)
    hist = R.histogram(y, cluster, v, N_BINS)
    assert torch.equal(voxel.group_histogram(y_dev, g, N_BINS).cpu(), hist)
    votes = voxel.group_vote(y_dev, g).cpu()
    assert votes.dtype == torch.int64
    assert torch.equal(votes, R.histogram(y, cluster, v, int(y.max()) + 1).argmax(dim=-1))
    flags = y % 2 == 0
    assert torch.equal(voxel.group_vote(flags.to(dev), g).cpu(),
                       R.histogram(flags.int(), cluster, v, 2).argmax(dim=-1))
    # integer means floor, like scatter_mean
    assert torch.equal(voxel.group_mean(y_dev, g).cpu(), R.scatter_mean(y, cluster, v))
    # a wide label range (super_index): the relabelling route, same rule
    wide = (torch.arange(n) * 37) % 300
    assert torch.equal(voxel.group_vote(wide.to(dev), g).cpu(),
                       R.histogram(wide, cluster, v, int(wide.max()) + 1).argmax(dim=-1))


def test_every_point_its_own_voxel(dev):
    from superpoint_transformer_amd import voxel
    n = 1000
    i = torch.arange(n)
    pos = torch.stack(((i % 10) * 1.0, ((i // 10) % 10) * 1.0, (i // 100) * 1.0), dim=1)[torch.randperm(n)]
    g = voxel.voxel_groups(pos.to(dev), 0.5)
    cluster, v = check_groups(g, pos, 0.5)
    assert v == n
    x = torch.randn(n, 3)
    assert torch.equal(voxel.group_mean(x.to(dev), g).cpu(), x[g.last.cpu()])


def test_one_voxel_of_70000_points(dev):
    """One run across many sort tiles and workgroups; the wave-parallel paths of every reduce."""
    from superpoint_transformer_amd import voxel
    n = 70_000
    pos = (torch.rand(n, 3) - 0.5) * 0.9            # all inside the voxel at the origin, size 1
    g = voxel.voxel_groups(pos.to(dev), 1.0)
    cluster, v = check_groups(g, pos, 1.0)
    assert v == 1 and int(g.last) == n - 1
    x = torch.randn(n, 3) + 5
    a = check_mean(x.to(dev), x, g, cluster, v)
    assert torch.equal(a, voxel.group_mean(x.to(dev), g).cpu())      # fixed tree: bitwise stable
    y = labels_for(n, N_BINS, 3)
    assert torch.equal(voxel.group_histogram(y.to(dev), g, N_BINS).cpu(), R.histogram(y, cluster, v, N_BINS))
    tie = torch.where(torch.arange(n) % 2 == 0, 7, 3)               # 35 000 each: the lowest wins
    assert voxel.group_vote(tie.to(dev), g).cpu().tolist() == [3]
    a, b = voxel.group_last(g, seed=11), voxel.group_last(g, seed=11)
    assert torch.equal(a, b) and 0 <= int(a) < n
    assert int(voxel.group_last(g, seed=12)) != int(a) or int(voxel.group_last(g, seed=13)) != int(a)


def test_run_lengths_at_the_path_thresholds(dev):
    """Voxels of exactly 16 / 17 points (the vote's lane and wave paths) and 512 / 513 points (the
    lane and wave paths of mean, histogram and representative), side by side."""
    from superpoint_transformer_amd import voxel
    sizes = (16, 17, 512, 513, 1)
    pos = torch.cat([(torch.rand(k, 3) - 0.5) * 0.9 + torch.tensor([3.0 * i, 0.0, 0.0])
                     for i, k in enumerate(sizes)])
    n = pos.shape[0]
    perm = torch.randperm(n)
    pos = pos[perm]
    g = voxel.voxel_groups(pos.to(dev), 1.0)
    cluster, v = check_groups(g, pos, 1.0)
    assert sorted(torch.bincount(cluster).tolist()) == sorted(sizes)
    x = torch.randn(n, 3) * 2 + 7
    check_mean(x.to(dev), x, g, cluster, v)
    check_mean(x[:, 0].to(dev), x[:, 0], g, cluster, v)
    y = labels_for(n, N_BINS, 4)
    assert torch.equal(voxel.group_histogram(y.to(dev), g, N_BINS).cpu(), R.histogram(y, cluster, v, N_BINS))
    two = torch.arange(n) % 2 * 5 + 3                                 # labels 3 and 8, near ties
    for labels in (y, two):
        want = R.histogram(labels, cluster, v, int(labels.max()) + 1).argmax(dim=-1)
        assert torch.equal(voxel.group_vote(labels.to(dev), g).cpu(), want)
    cpu_groups = voxel.voxel_groups(pos, 1.0)
    for seed in (0, 3, 2 ** 63 + 5):
        rep = voxel.group_last(g, seed=seed).cpu()
        assert torch.equal(cluster[rep], torch.arange(v))
        assert torch.equal(rep, voxel.group_last(cpu_groups, seed=seed))   # the same stream on the CPU


def test_key_wider_than_32_bits(dev):
    """Two clusters 30 km apart at 3 cm: about 20 bits per horizontal axis, the sort's second word."""
    from superpoint_transformer_amd import voxel
    n = 4000
    pos = cloud(n, 0.03, seed=5)
    pos[n // 2:] += torch.tensor([30_000.0, 30_000.0, 100.0])
    pos = pos[torch.randperm(n)]
    g = voxel.voxel_groups(pos.to(dev), 0.03)
    coords = torch.round(pos / 0.03).long()
    bits = sum(int(c.max() - c.min()).bit_length() for c in coords.T)
    assert bits > 32
    cluster, v = check_groups(g, pos, 0.03)
    x = torch.randn(n, 3)
    check_mean(x.to(dev), x, g, cluster, v)


def test_clouds_with_identical_coordinates_and_different_batch(dev):
    from superpoint_transformer_amd import voxel
    one = cloud(700, 0.05, seed=9)
    pos = torch.cat([one, one, one])
    batch = torch.arange(3).repeat_interleave(700)
    perm = torch.randperm(2100)
    pos, batch = pos[perm], batch[perm]
    g = voxel.voxel_groups(pos.to(dev), 0.05, batch.to(dev))
    cluster, v = check_groups(g, pos, 0.05, batch)
    g1 = voxel.voxel_groups(one.to(dev), 0.05)
    assert v == 3 * g1.num_voxels
    assert torch.equal(batch[g.last.cpu()], torch.arange(3).repeat_interleave(g1.num_voxels))


def test_bad_inputs_raise_before_any_kernel_indexes_with_them(dev):
    from superpoint_transformer_amd import voxel
    pos = cloud(500, 0.05, seed=2)
    g = voxel.voxel_groups(pos.to(dev), 0.05)
    y = labels_for(500, N_BINS, 2)
    y[17] = N_BINS                                                   # a label equal to n_bins
    with pytest.raises(ValueError):
        voxel.group_histogram(y.to(dev), g, N_BINS)
    y[17] = -1
    with pytest.raises(ValueError):
        voxel.group_histogram(y.to(dev), g, N_BINS)
    with pytest.raises(ValueError):
        voxel.group_vote(y.to(dev), g)
    bad = pos.clone()
    bad[100, 2] = float("nan")
    with pytest.raises(ValueError):
        voxel.voxel_groups(bad.to(dev), 0.05)
    bad[100, 2] = float("inf")
    with pytest.raises(ValueError):
        voxel.voxel_groups(bad.to(dev), 0.05)
    far = torch.tensor([[-3000.0] * 3, [3000.0] * 3])                # 23 bits per axis at 1 mm
    with pytest.raises(ValueError, match="bits"):
        voxel.voxel_groups(far.to(dev), 1e-3)
    with pytest.raises(ValueError):
        voxel.voxel_groups(far.to(dev), 1e-9)                        # beyond 32 bits per axis


def test_vote_ties_go_to_the_lowest_label(dev):
    from superpoint_transformer_amd import voxel
    # voxel 0: labels 5 2 5 2 (tie); voxel 1: 20 points, 9 9 ... 4 4 ... tied (the wave path)
    pos = torch.cat([torch.zeros(4, 3), torch.ones(20, 3)])
    y = torch.cat([torch.tensor([5, 2, 5, 2]), torch.tensor([9, 4]).repeat(10)])
    g = voxel.voxel_groups(pos.to(dev), 0.5)
    assert voxel.group_vote(y.to(dev), g).cpu().tolist() == [2, 4]


def test_transform_on_the_device(dev):
    """The whole transform on a generated cloud: sub, obj, DataTo, mode='last'."""
    from superpoint_transformer_amd import voxel
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import DataTo, GridSampling3D, SaveNodeIndex
    n = 5000
    pos = cloud(n, 0.05, seed=21, per_voxel=4.0)
    y = labels_for(n, N_BINS, 21)
    obj = (torch.arange(n) * 13) % 29
    raw = Data(pos=pos, rgb=torch.rand(n, 3), obj=obj, y=y)
    data = SaveNodeIndex(key="sub")(DataTo(dev)(raw))
    assert data is not raw and data.pos.is_cuda and raw.pos.device.type == "cpu"
    t = GridSampling3D(0.05, hist_key="y", hist_size=N_BINS, inplace=True)
    out = t(data)
    g = t.groups_
    assert out is data and torch.equal(out.sub.to_super_index(), g.cluster)
    assert torch.equal(out.sub.pointers, g.pointers) and out.sub.ascending
    fields = dict(pos=pos, rgb=raw.rgb, obj=obj, y=y, sub=torch.arange(n))
    want = R.grid_sampling(fields, 0.05, hist_key="y", hist_size=N_BINS)
    for got, ref in zip((out.obj.pointers, out.obj.obj, out.obj.count, out.obj.y), want["obj"]):
        assert torch.equal(got.cpu(), ref)
    assert torch.equal(out.y.cpu(), want["y"])
    assert R.bits_equal(out.pos.cpu().numpy(), want["pos"].numpy())
    assert R.bits_equal(out.rgb.cpu().numpy(), want["rgb"].numpy())

    # mode='last': the representative lies in its voxel, follows torch's seed, differs between seeds
    def last(seed):
        torch.manual_seed(seed)
        d = Data(pos=pos.to(dev), node_id=torch.arange(n, device=dev))
        return GridSampling3D(0.05, mode="last")(d).node_id

    a, b, c = last(1), last(1), last(2)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(g.cluster[a], torch.arange(g.num_voxels, device=dev))
    assert torch.equal(voxel.group_last(g, seed=None), g.last)
    cpu_groups = voxel.voxel_groups(pos, 0.05)
    assert torch.equal(voxel.group_last(g, seed=99).cpu(), voxel.group_last(cpu_groups, seed=99))


@pytest.mark.parametrize("n,two_words", [(65, False), (9000, False), (9000, True)])
def test_workspaces_are_exact_size(n, two_words, dev):
    """Every scratch request gets exactly the bytes the entry's query promised, between guards."""
    from superpoint_transformer_amd import voxel
    pos = cloud(n, 0.03, seed=n)
    if two_words:
        pos[n // 2:] += torch.tensor([30_000.0, 30_000.0, 0.0])
    arena = GuardedArena(dev)
    with exact_workspaces(arena):
        g = voxel.voxel_groups(pos.to(dev), 0.03)
        torch.cuda.synchronize()
    assert len(arena) >= 1
    check_groups(g, pos, 0.03)
