"""The entries of csrc/panoptic.hip under tests/guarded.py, called through the C ABI: every input
flush against its guard (NaN behind floats, zero behind indices), every output and in-place
operand cut to the byte between guards and pre-filled with a sentinel, the workspace exactly
what its query promises and NaN-filled (0xFF: -1 as an index, NaN as a float).  Asked for: intact
guards and the bits of the plain run through the Python wrappers."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc
from guarded import GuardedArena

pytestmark = pytest.mark.gpu

SENTINEL = -7777


def arena_for(dev):
    return GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)


def put(arena, t, label):
    return arena.place(t, guard_byte=0xFF if t.is_floating_point() else 0x00, label=label)


def fresh(arena, n, dtype, label, fill=SENTINEL):
    t = arena.take(n * torch.empty((), dtype=dtype).element_size(), dtype, (n,), label)
    if dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(fill)
    return t


def call(name, *args):
    from superpoint_transformer_amd import _lib
    dev = torch.cuda.current_device()
    st = getattr(_lib.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                 _lib.stream_ptr(dev))
    _lib.check(st, name)


def query(name, *args):
    from superpoint_transformer_amd import _lib
    return getattr(_lib.lib, name)(*args)


def bits_for(n):
    return max(1, (int(n) - 1).bit_length())


def test_wrappers_on_exact_poisoned_memory(dev):
    """The whole Python surface once more with every ``_workspace`` request cut to the byte
    between guards and NaN-filled, and every fresh float tensor NaN-filled: the comparisons
    with the reference's fixture must hold unchanged."""
    from guarded import exact_workspaces, poisoned_fresh_tensors
    arena = arena_for(dev)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        pc.check_merge(dev)
        pc.check_stats(dev)
        pc.check_output(dev)
        pc.check_big_mean(dev)
        for variant in sorted(pc.VARIANTS):
            (two, one), _ = pc.check_metric(dev, variant)
            assert two == one
    assert len(arena) > 0


CASES = [(1, 1, 1), (17, 70, 1), (257, 1, 1 << 33), (700, 3, 1)]


def placed(arena, d):
    return [put(arena, t, k) for t, k in ((d.pointers, "pointers"), (d.obj, "obj"),
                                          (d.count, "count"), (d.y, "y"))]


@pytest.mark.parametrize("g,per_cluster,spread", CASES)
def test_merge_instances_between_guards(g, per_cluster, spread, dev):
    from superpoint_transformer_amd import panoptic
    d = pc.random_instance(g, per_cluster, 13, seed=g, spread=spread).to(dev)
    rng = np.random.default_rng(g)
    k = max(1, g // 4)
    idx = rng.integers(0, k, g)
    idx[:k] = np.arange(k)
    idx = torch.from_numpy(idx).to(dev)
    want = panoptic.merge_instances(d, idx)
    p, lo, hi = d.num_items, *want._obj_extent
    arena = arena_for(dev)
    ext = fresh(arena, 4, torch.int64, "extents")
    ptr, obj, count, y = placed(arena, d)
    didx = put(arena, idx, "idx")
    call("spt_instance_extents_i64", obj, p, didx, g, ext)
    arena.check()
    assert ext.tolist() == [lo, hi, 0, k - 1]
    obj_bits = bits_for(hi - lo + 1)
    nbytes = query("spt_merge_instances_workspace_bytes", p, obj_bits + bits_for(k))
    ws = arena.take(nbytes, label="ws")
    out_ptr = fresh(arena, k + 1, torch.int64, "out_pointers")
    out = [fresh(arena, p, torch.int64, n) for n in ("out_obj", "out_count", "out_y")]
    rec = put(arena, torch.zeros(4, dtype=torch.int64, device=dev), "record")
    call("spt_merge_instances_i64", ptr, obj, count, y, didx, g, p, k, lo, obj_bits, out_ptr,
         *out, rec, ws, nbytes)
    arena.check()
    r = want.num_items
    assert rec.tolist() == [r, k, 0, 0]
    assert torch.equal(out_ptr, want.pointers)
    for got, exp in zip(out, (want.obj, want.count, want.y)):
        assert torch.equal(got[:r], exp) and bool((got[r:] == SENTINEL).all())


@pytest.mark.parametrize("g,per_cluster,spread", CASES)
def test_pair_stats_and_counts_between_guards(g, per_cluster, spread, dev):
    from superpoint_transformer_amd import panoptic
    c = 13
    d = pc.random_instance(g, per_cluster, c, seed=7 * g, spread=spread).to(dev)
    d.pair_cropped_count = torch.arange(d.num_items, device=dev) % 5
    p = d.num_items
    pred = torch.from_numpy(np.random.default_rng(g).integers(-1, c + 1, g)).to(dev)
    stuff = (torch.arange(c, device=dev) < 3)
    want = panoptic.pair_stats(d, c)
    state = panoptic.new_state(c, dev) + 3
    state[3:] = 0
    panoptic.panoptic_counts_(state, pred, d, c, stuff, stats=want)

    arena = arena_for(dev)
    ptr, obj, count, y = placed(arena, d)
    crop_in = put(arena, d.pair_cropped_count, "cropped_in")
    nbytes = query("spt_pair_stats_workspace_bytes", p, g, 63)
    ws = arena.take(nbytes, label="ws")
    a_size, b_size, crop = (fresh(arena, p, torch.int64, n) for n in ("a_size", "b_size", "cropped"))
    iou, kept = fresh(arena, p, torch.float32, "iou"), fresh(arena, p, torch.float32, "kept_iou")
    cl_void = fresh(arena, g, torch.uint8, "cluster_void", fill=7)
    p_void, head = (fresh(arena, p, torch.uint8, n, fill=7) for n in ("pair_void", "gt_head"))
    status = put(arena, torch.zeros(4, dtype=torch.int32, device=dev), "status")
    call("spt_pair_stats_i64", ptr, obj, count, y, crop_in, g, p, c, 0, 63, a_size, b_size, iou,
         cl_void, p_void, crop, kept, head, status, ws, nbytes)
    arena.check()
    for got, exp in ((a_size, want.a_size), (b_size, want.b_size), (crop, want.pair_cropped_count),
                     (cl_void, want.is_cluster_void), (p_void, want.is_pair_void),
                     (head, want.gt_head)):
        assert torch.equal(got, exp.to(got.dtype))
    assert pc.bits(iou) == pc.bits(want.iou) and pc.bits(kept) == pc.bits(want.kept_iou)
    assert status.tolist() == [0, 0, 0, 0]

    nb2 = query("spt_panoptic_counts_workspace_bytes", c)
    ws2 = arena.take(nb2, label="counts ws")
    st = fresh(arena, 5 * c, torch.int64, "state", fill=3)
    st[3 * c:] = 0
    dpred, dstuff = put(arena, pred, "pred"), put(arena, stuff.to(torch.uint8), "stuff")
    call("spt_panoptic_counts_i64", st, dpred, ptr, y, p_void, kept, head, cl_void, g, p, c,
         dstuff, status, ws2, nb2)
    arena.check()
    assert pc.bits(st) == pc.bits(state)
    assert status.tolist() == want.status.tolist()


@pytest.mark.parametrize("n,groups,cols", [(1, 1, 1), (65, 17, 13), (1729, 6, 13), (3000, 300, 33)])
def test_weighted_group_mean_between_guards(n, groups, cols, dev):
    from superpoint_transformer_amd import panoptic
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(size=(n, cols)).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.integers(0, groups, n)).to(dev)
    if n == 1729:                                          # the fixture's 512 / 513 / 700 runs
        idx = pc.T("big__in__idx", dev)
    if n > 10:
        idx[3], idx[9] = groups, -1                        # out of range: left out, counted
    w = torch.from_numpy(rng.integers(0, 40, n).astype(np.float32)).to(dev)
    want = panoptic.weighted_group_mean(x, idx, w, groups, check=False)
    arena = arena_for(dev)
    dx, di, dw = put(arena, x, "x"), put(arena, idx, "idx"), put(arena, w, "w")
    nbytes = query("spt_weighted_group_mean_workspace_bytes", n, groups)
    ws = arena.take(nbytes, label="ws")
    out = fresh(arena, groups * cols, torch.float32, "out")
    status = put(arena, torch.zeros(2, dtype=torch.int32, device=dev), "status")
    call("spt_weighted_group_mean_f32", dx, n, cols, di, dw, groups, out, status, ws, nbytes)
    arena.check()
    assert pc.bits(out) == pc.bits(want) and not bool(out.isnan().any())
    assert status.tolist() == [2 if n > 10 else 0, 0]
