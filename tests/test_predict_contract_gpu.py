"""The four entries of csrc/predict.hip under tests/guarded.py, called through the C ABI:
every input flush against its guard (NaN behind floats, zero behind indices: a stray index reads
0, in range, and shows in the result), every output and in-place operand cut to the byte between
guards and pre-filled with a sentinel, so that an element nobody wrote shows.  Out-of-range
inputs are part of the cases: the kernels' own bounds checks must leave every guard intact."""
import numpy as np
import pytest
import torch

from guarded import GuardedArena

pytestmark = pytest.mark.gpu

SENTINEL = -7777


def arena_for(dev):
    return GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)


def put(arena, t, label):
    return arena.place(t, guard_byte=0xFF if t.is_floating_point() else 0x00, label=label)


def fresh(arena, n, dtype, label, fill=SENTINEL):
    t = arena.take(n * torch.empty((), dtype=dtype).element_size(), dtype, (n,), label)
    t.fill_(fill)
    return t


def call(name, *args):
    from superpoint_transformer_amd import _lib
    dev = torch.cuda.current_device()
    st = getattr(_lib.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                 _lib.stream_ptr(dev))
    _lib.check(st, name)


@pytest.mark.parametrize("rows,c", [(1, 1), (65, 13), (1000, 33)])
def test_row_argmax_between_guards(rows, c, dev):
    arena = arena_for(dev)
    gen = torch.Generator().manual_seed(rows)
    z = (torch.randn(rows, c, generator=gen) * 2).round() / 2
    z[rows // 2, c // 2] = float("nan")
    h = torch.randint(0, 9, (rows, c + 1), generator=gen)
    h[0] = 0
    dz, dh = put(arena, z.to(dev), "logits"), put(arena, h.to(dev), "hist")
    pred = fresh(arena, rows, torch.int64, "pred")
    void = fresh(arena, rows, torch.uint8, "is_void", fill=7)
    call("spt_row_argmax_f32", dz, rows, c, dh, c + 1, pred, void)
    arena.check()
    assert torch.equal(pred.cpu(), torch.argmax(z, dim=1))
    assert torch.equal(void.cpu().bool(), h[:, -1] / h.sum(dim=1) > 0.5) and int(void.max()) <= 1
    # either half alone
    pred.fill_(SENTINEL)
    call("spt_row_argmax_f32", dz, rows, c, None, 0, pred, None)
    void.fill_(7)
    call("spt_row_argmax_f32", None, rows, 0, dh, c + 1, None, void)
    arena.check()
    assert torch.equal(pred.cpu(), torch.argmax(z, dim=1)) and int(void.max()) <= 1


@pytest.mark.parametrize("n,c", [(1, 1), (65, 13), (300, 33)])
def test_rows_accumulate_between_guards(n, c, dev):
    N = 300
    arena = arena_for(dev)
    gen = torch.Generator().manual_seed(n)
    base = torch.randn(N, c, generator=gen)
    src = torch.randn(n, c, generator=gen)
    ids = torch.randperm(N, generator=gen)[:n]
    if n > 10:
        ids[5], ids[6], ids[7] = N, -1, ids[0]               # past the end, negative, a duplicate
    acc, dsrc = put(arena, base.to(dev), "acc"), put(arena, src.to(dev), "src")
    dids = put(arena, ids.to(dev), "node_id")
    stamp = put(arena, torch.zeros(N, dtype=torch.int32, device=dev), "stamp")
    status = put(arena, torch.zeros(2, dtype=torch.int32, device=dev), "status")
    call("spt_rows_accumulate_f32", acc, N, dsrc, dids, n, c, stamp, 1, status)
    arena.check()
    ok = torch.ones(n, dtype=torch.bool)
    if n > 10:
        ok[[0, 5, 6, 7]] = False
    want = base.clone()
    want[ids[ok]] += src[ok]
    got = acc.cpu()
    rest = torch.ones(N, dtype=torch.bool)
    if n > 10:
        twice = int(ids[0])
        rest[twice] = False
        assert torch.equal(got[twice], base[twice] + src[0]) or torch.equal(got[twice], base[twice] + src[7])
        assert status.tolist() == [1, 2]
    else:
        assert status.tolist() == [0, 0]
    assert got[rest].numpy().tobytes() == want[rest].numpy().tobytes()
    want_stamp = torch.zeros(N, dtype=torch.int32)
    want_stamp[ids[(ids >= 0) & (ids < N)]] = 1
    assert torch.equal(stamp.cpu(), want_stamp)


def small_hierarchy(n_raw, seed):
    rng = np.random.default_rng(seed)
    n_vox, n_sp = max(1, n_raw // 4), max(1, n_raw // 32)
    label = torch.from_numpy(rng.integers(0, 13, n_sp))
    si01 = torch.from_numpy(rng.integers(0, n_sp, n_vox))
    si_raw0 = torch.from_numpy(rng.integers(0, n_vox, n_raw))
    si_raw0[-1] = n_vox - 1
    order = torch.sort(si_raw0, stable=True).indices
    sizes = torch.bincount(si_raw0, minlength=n_vox)
    ptr = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    pts = order.clone()
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        pts[a:b] = pts[a:b][torch.from_numpy(rng.permutation(b - a))]
    y = torch.from_numpy(rng.integers(-1, 15, n_raw))
    return label, si01, si_raw0, ptr, pts, y


@pytest.mark.parametrize("n_raw", [1, 257, 1025, 2500])
def test_labels_by_index_between_guards(n_raw, dev):
    from superpoint_transformer_amd import ops
    label, si01, si_raw0, _, _, y = small_hierarchy(n_raw, n_raw)
    n_sp, n_vox = label.numel(), si01.numel()
    if n_raw > 100:
        si01[3], si01[9] = n_sp, -1                          # out of range: -1, counted
        si_raw0[11], si_raw0[12] = n_vox, -5
    want_v = label[si01.clamp(0, n_sp - 1)]
    want_v[(si01 < 0) | (si01 >= n_sp)] = -1
    want_r = want_v[si_raw0.clamp(0, n_vox - 1)]
    want_r[(si_raw0 < 0) | (si_raw0 >= n_vox)] = -1
    want_cm = ops.histogram_confusion_matrix(want_r, y, 13) + 2
    arena = arena_for(dev)
    dl, da, db, dy = (put(arena, t.to(dev), k) for t, k in
                      ((label, "label"), (si01, "idx_a"), (si_raw0, "idx_b"), (y, "target")))
    out_a, out_b = fresh(arena, n_vox, torch.int64, "out_a"), fresh(arena, n_raw, torch.int64, "out_b")
    cm = fresh(arena, 13 * 13, torch.int64, "confmat", fill=2)
    status = put(arena, torch.zeros(4, dtype=torch.int32, device=dev), "status")
    call("spt_labels_by_index_i64", dl, n_sp, da, n_vox, db, n_raw, out_a, out_b, dy, 13, cm, status)
    arena.check()
    assert torch.equal(out_a.cpu(), want_v) and torch.equal(out_b.cpu(), want_r)
    assert torch.equal(cm.cpu().view(13, 13), want_cm)
    assert status.tolist() == ([2, 2, 0, 0] if n_raw > 100 else [0, 0, 0, 0])
    # the evaluation case: both outputs null, nothing but the matrix and the status is written
    cm.fill_(2)
    call("spt_labels_by_index_i64", dl, n_sp, da, n_vox, db, n_raw, None, None, dy, 13, cm, status)
    arena.check()
    assert torch.equal(cm.cpu().view(13, 13), want_cm)


@pytest.mark.parametrize("n_raw", [1, 257, 1025, 2500])
def test_labels_by_cluster_between_guards(n_raw, dev):
    from superpoint_transformer_amd import ops
    label, si01, si_raw0, ptr, pts, y = small_hierarchy(n_raw, 3 * n_raw)
    n_sp, n_vox = label.numel(), si01.numel()
    unwritten = []
    if n_raw > 100:
        si01[3], si01[9] = n_sp, -1
        unwritten = [int(pts[20]), int(pts[n_raw - 1])]
        pts[20], pts[n_raw - 1] = n_raw, -1                  # never written through
    want_v = label[si01.clamp(0, n_sp - 1)]
    want_v[(si01 < 0) | (si01 >= n_sp)] = -1
    want_r = want_v[si_raw0]
    cm_pred = want_r.clone()
    if unwritten:
        want_r[unwritten] = SENTINEL
        cm_pred[unwritten] = -1
    want_cm = ops.histogram_confusion_matrix(cm_pred, y, 13) + 2
    arena = arena_for(dev)
    dl, da, dp, dq, dy = (put(arena, t.to(dev), k) for t, k in
                          ((label, "label"), (si01, "idx_a"), (ptr, "pointers"), (pts, "points"),
                           (y, "target")))
    out = fresh(arena, n_raw, torch.int64, "out")
    cm = fresh(arena, 13 * 13, torch.int64, "confmat", fill=2)
    status = put(arena, torch.zeros(4, dtype=torch.int32, device=dev), "status")
    call("spt_labels_by_cluster_i64", dl, n_sp, da, dp, dq, n_vox, n_raw, out, dy, 13, cm, status)
    arena.check()
    assert torch.equal(out.cpu(), want_r)
    assert torch.equal(cm.cpu().view(13, 13), want_cm)
    assert status.tolist() == ([2, 2, 0, 0] if n_raw > 100 else [0, 0, 0, 0])
    # without the first-hop index (labels per cluster), output null: the matrix alone
    cm.fill_(2)
    dv = put(arena, want_v.to(dev), "voxel labels")
    call("spt_labels_by_cluster_i64", dv, n_vox, None, dp, dq, n_vox, n_raw, None, dy, 13, cm, status)
    arena.check()
    assert torch.equal(cm.cpu().view(13, 13), want_cm)
