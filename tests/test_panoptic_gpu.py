"""The panoptic evaluation on the device: the comparisons of tests/panoptic_cases.py against the
reference's fixture, then the shapes at which the kernels of csrc/panoptic.hip can go wrong, each
against the CPU route (exact: integers, IoU bits, state bits - the float sums are fixed-point
integers on both routes).  Float bars: tests/panoptic_cases.py; measured figures:
profiles/r19a_panoptic_errors.txt."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc

pytestmark = pytest.mark.gpu


def test_merge_instances_exact(dev):
    pc.check_merge(dev)


def test_pair_stats_exact_and_iou_bit_for_bit(dev):
    pc.check_stats(dev)


def test_output_surface(dev):
    pc.check_output(dev)


def test_weighted_mean_at_and_past_the_sequential_limit(dev):
    pc.check_big_mean(dev)


@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_metric_matches_reference_and_cpu_route(variant, dev):
    (two, one), _ = pc.check_metric(dev, variant)
    assert two == one                                   # two updates == one batch update
    (cpu_two, _), _ = pc.check_metric("cpu", variant)
    assert two[0] == cpu_two[0]                         # the state, bit for bit


def test_host_reads(dev):
    """None in update, one in compute, two in merge_instances."""
    reads = []
    real = torch.Tensor.tolist
    real_item, real_cpu = torch.Tensor.item, torch.Tensor.cpu

    def counted(name, fn):
        def wrapper(self, *a, **k):
            if self.is_cuda:
                reads.append(name)
            return fn(self, *a, **k)
        return wrapper
    from superpoint_transformer_amd import panoptic
    d, idx = pc.instance("l1", dev), pc.T("in__idx1", dev)
    m, pred = pc.instance("m1", dev), pc.T("obj_y", dev)
    pq = pc.metric(dev, "pq", True)
    pq.reset()
    torch.Tensor.tolist = counted("tolist", real)
    torch.Tensor.item = counted("item", real_item)
    torch.Tensor.cpu = counted("cpu", real_cpu)
    try:
        panoptic.merge_instances(d, idx)
        assert len(reads) == 2, reads
        del reads[:]
        pq.update(pred, m)
        assert reads == [], reads
        pq.compute()
        assert len(reads) == 1, reads
    finally:
        torch.Tensor.tolist, torch.Tensor.item, torch.Tensor.cpu = real, real_item, real_cpu


# ---- shapes --------------------------------------------------------------------------------------
def same_data(a, b):
    for k in ("pointers", "obj", "count", "y"):
        assert torch.equal(getattr(a, k).cpu(), getattr(b, k).cpu()), k


def same_stats(a, b):
    for k in ("a_size", "b_size", "is_cluster_void", "is_pair_void", "pair_cropped_count", "gt_head"):
        assert torch.equal(getattr(a, k).cpu(), getattr(b, k).cpu()), k
    for k in ("iou", "kept_iou"):
        assert pc.bits(getattr(a, k)) == pc.bits(getattr(b, k)), k
    assert a.status.tolist() == b.status.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("g", [1, 17, 257, 16 * 131 + 5])
@pytest.mark.parametrize("per_cluster", [1, 70])
def test_shapes_against_cpu_route(g, per_cluster, dev):
    from superpoint_transformer_amd import panoptic
    c = {1: 1, 17: 13, 257: 32}.get(g, 13)
    spread = (1 << 33) if g == 257 else 1                 # a key needing more than 32 bits
    d = pc.random_instance(g, per_cluster, c, seed=g * 100 + per_cluster, spread=spread)
    rng = np.random.default_rng(g)
    parents = {"one": np.zeros(g, dtype=np.int64), "own": rng.permutation(g)}
    if g > 1:
        k = max(2, g // 5)
        mixed = rng.integers(0, k, g)
        mixed[:k] = np.arange(k)
        parents["mixed"] = mixed
    stuff = torch.zeros(c, dtype=torch.bool)
    stuff[: c // 3] = True                                # (none for c = 1)
    for name, idx in parents.items():
        idx = torch.from_numpy(idx)
        want = panoptic.merge_instances(d, idx)
        got = panoptic.merge_instances(d.to(dev), idx.to(dev))
        same_data(got, want)
        if spread > 1:
            lo, hi = got._obj_extent
            assert (hi - lo).bit_length() + (int(idx.max())).bit_length() > 32
        pred = torch.from_numpy(rng.integers(0, c, want.num_groups))
        states = []
        for data, where in ((want, "cpu"), (got, dev), (got, dev)):
            s = panoptic.pair_stats(data, c)
            state = panoptic.new_state(c, where)
            panoptic.panoptic_counts_(state, pred.to(where), data, c, stuff.to(where), stats=s)
            states.append((s, pc.bits(state)))
        same_stats(states[1][0], states[0][0])
        same_stats(states[2][0], states[1][0])            # two calls: identical bits
        assert states[0][1] == states[1][1] == states[2][1], name
        assert states[0][0].status.tolist() == [0, 0, 0, 0]
        # without the extents merge_instances left behind: the 63-bit object sort
        plain = type(got)(got.pointers, got.obj, got.count, got.y)
        same_stats(panoptic.pair_stats(plain, c), states[0][0])


def test_runs_past_512_take_the_whole_wave(dev):
    """1 500 clusters that all overlap object 7 (and one object of their own): the run of that
    object, the run of the (parent 0, object 7) key and the merged cluster of 1 501 pairs are
    reduced by a whole wave; a second long run sits next to it, a void one."""
    from superpoint_transformer_amd import panoptic
    from superpoint_transformer_amd.instance import InstanceData
    g, c = 1500, 13
    rng = np.random.default_rng(5)
    own = 10 + 3 * np.arange(g)
    shared = np.where(np.arange(g) % 2 == 0, 7, 8)
    shared[:600] = 7                                          # 1 050 clusters on 7, 450 on 8
    obj = np.stack((shared, own), axis=1).reshape(-1)
    y = np.stack((np.where(shared == 7, 2, -1), rng.integers(0, c, g)), axis=1).reshape(-1)
    count = rng.integers(1, 90, 2 * g)
    T = torch.from_numpy
    d = InstanceData(T(np.arange(g + 1) * 2), T(obj), T(count), T(y))
    stuff = torch.arange(c) < 3
    for idx in (torch.zeros(g, dtype=torch.long), torch.arange(g) % 2):
        want = panoptic.merge_instances(d, idx)
        got = panoptic.merge_instances(d.to(dev), idx.to(dev))
        same_data(got, want)
        for data_cpu, data_dev in ((want, got), (d, d.to(dev))):
            pred = T(rng.integers(0, c, data_cpu.num_groups))
            a, b = panoptic.pair_stats(data_cpu, c), panoptic.pair_stats(data_dev, c)
            same_stats(b, a)
            sa, sb = panoptic.new_state(c), panoptic.new_state(c, dev)
            panoptic.panoptic_counts_(sa, pred, data_cpu, c, stuff, stats=a)
            panoptic.panoptic_counts_(sb, pred.to(dev), data_dev, c, stuff.to(dev), stats=b)
            assert pc.bits(sa) == pc.bits(sb)


@pytest.mark.parametrize("n,groups", [(1, 1), (65, 17), (5000, 257), (3000, 1)])
def test_weighted_mean_against_cpu_route(n, groups, dev):
    """Groups up to the sequential limit: the CPU route's bits; one group of 3 000 rows (64 lanes
    of 47 rows and a tree): within the worst-case bound of that summation, stated below."""
    from superpoint_transformer_amd import panoptic
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(size=(n, 13)).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, groups, n))
    w = torch.from_numpy(rng.integers(0, 40, n))
    want = panoptic.weighted_group_mean(x, idx, w, groups + 1)       # the last group has no row
    a = panoptic.weighted_group_mean(x.to(dev), idx.to(dev), w.to(dev), groups + 1)
    b = panoptic.weighted_group_mean(x.to(dev), idx.to(dev), w.to(dev), groups + 1)
    assert pc.bits(a) == pc.bits(b) and not a[groups].any()
    if int(torch.bincount(idx).max()) <= panoptic.SEQUENTIAL_ROWS:
        assert pc.bits(a) == pc.bits(want)
    else:
        wd = w.double().view(-1, 1)
        f64 = (x.double() * wd).sum(0) / wd.sum()
        # each term passes one product rounding, at most 47 adds in its lane, 6 in the tree and
        # the division; the weight sum as many: (1 + 47 + 6 + 1) * 2 units of 2^-24 of sum |term|
        bound = 110 * 2.0 ** -24 * (x.double().abs() * wd).sum(0) / wd.sum()
        assert ((a[0].cpu().double() - f64).abs() <= bound).all()
    x1 = x[:, 0].contiguous()                                         # a 1-D x is [N, 1]
    assert pc.bits(panoptic.weighted_group_mean(x1.to(dev), idx.to(dev), w.to(dev), groups + 1)) \
        == pc.bits(a[:, :1].contiguous())


def test_faults_are_counted_not_followed(dev):
    from superpoint_transformer_amd import panoptic
    from superpoint_transformer_amd.instance import InstanceData
    d = pc.instance("l1", dev)
    idx = pc.T("in__idx1", dev)
    broken = InstanceData(d.pointers.clone(), d.obj, d.count, d.y)
    broken.pointers[-1] -= 1
    with pytest.raises(ValueError, match="pointers"):
        panoptic.merge_instances(broken, idx)
    gap = idx.clone()
    gap[gap == 4] = 3
    with pytest.raises(AssertionError, match="Indices must be dense"):
        panoptic.merge_instances(d, gap)
    with pytest.raises(AssertionError, match="contiguous indices"):
        panoptic.merge_instances(d, idx + 1)
    s = panoptic.pair_stats(broken, pc.C)
    assert s.status.tolist()[0] > 0
    x, i, w = torch.zeros(4, 3, device=dev), torch.tensor([0, 1, 5, -1], device=dev), \
        torch.ones(4, device=dev)
    with pytest.raises(ValueError, match="2 index entries outside"):
        panoptic.weighted_group_mean(x, i, w, 2)
    m = pc.instance("m1", dev)
    pq = pc.metric(dev, "pq", True)
    pq.reset()
    bad = pc.T("obj_y", dev).clone()
    bad[0] = pc.C
    pq.update(bad, m)
    with pytest.raises(ValueError, match="1 prediction"):
        pq.compute()
