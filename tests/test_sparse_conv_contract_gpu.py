"""The entries of csrc/sparse_conv.hip under tests/guarded.py, called through the C ABI: every
input flush against its guard (NaN behind floats, zero behind indices), every output cut to the
byte between guards, the workspace exactly what its query promises and NaN-filled.  Asked for:
intact guards and the bits of the plain run through the Python wrappers.  Then the wrappers
themselves on exact, poisoned scratch and poisoned fresh tensors."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_reference as R
from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors

pytestmark = pytest.mark.gpu


def arena_for(dev):
    return GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)


def put(arena, t, label):
    return arena.place(t, guard_byte=0xFF if t.is_floating_point() else 0x00, label=label)


def fresh(arena, shape, dtype, label):
    n = int(np.prod(shape))
    return arena.take(n * torch.empty((), dtype=dtype).element_size(), dtype, tuple(shape), label)


def call(name, *args):
    from superpoint_transformer_amd import _lib
    dev = torch.cuda.current_device()
    st = getattr(_lib.lib, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args],
                                 _lib.stream_ptr(dev))
    _lib.check(st, name)


def query(name, *args):
    from superpoint_transformer_amd import _lib
    return getattr(_lib.lib, name)(*args)


def _case(n, ci, co, K, seed, dev):
    coords, batch = R.random_cloud(n, 7, seed, batches=2)
    g = torch.Generator().manual_seed(seed)
    shape = (K ** 3, ci, co)
    x, W = torch.randn(n, ci, generator=g), torch.randn(shape, generator=g)
    b, gout = torch.randn(co, generator=g), torch.randn(n, co, generator=g)
    return coords.to(dev), batch.to(dev), x.to(dev), W.to(dev), b.to(dev), gout.to(dev)


def _plain(S, coords, batch, K, d, x, W, b, gout):
    kmap = S.build_kernel_map(coords, batch, K, d)
    xs, Ws, bs = (t.clone().requires_grad_() for t in (x, W, b))
    out = S.sparse_conv3d(xs, Ws, kmap, bs)
    out.backward(gout)
    return kmap, (out.detach(), xs.grad, Ws.grad, bs.grad)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n,ci,co,K,d", [(67, 3, 16, 3, 1), (130, 7, 32, 7, 2), (33, 32, 64, 1, 1)])
def test_entries_between_guards(n, ci, co, K, d, dev):
    from superpoint_transformer_amd import sparse as S
    coords, batch, x, W, b, gout = _case(n, ci, co, K, n, dev)
    kmap, want = _plain(S, coords, batch, K, d, x, W, b, gout)
    perm0, optr0 = kmap.by_offset()
    k3, P = K ** 3, kmap.num_pairs

    arena = arena_for(dev)
    c32 = put(arena, coords.int(), "coords")
    gb = put(arena, batch, "batch")
    # bounds
    record = fresh(arena, (8,), torch.int64, "bounds record")
    call("spt_sparse_bounds_i32", c32, gb, n, record)
    arena.check()
    rec = record.tolist()
    cc = coords.cpu()
    assert rec[0:6:2] == cc.min(0).values.tolist() and rec[1:6:2] == cc.max(0).values.tolist()
    assert rec[6:] == [0, 1]
    origin, bits, total = S._key_layout(rec[0:8:2], rec[1:8:2], (K // 2) * d)
    c_origin, c_bits = (ctypes.c_int64 * 4)(*origin), (ctypes.c_int * 4)(*bits)
    o_ptr, b_ptr = ctypes.addressof(c_origin), ctypes.addressof(c_bits)
    # count
    skeys = fresh(arena, (n,), torch.int64, "skeys")
    sorder = fresh(arena, (n,), torch.int32, "sorder")
    rowptr = fresh(arena, (n + 1,), torch.int32, "rowptr")
    record2 = fresh(arena, (2,), torch.int64, "pairs record")
    nbytes = query("spt_sparse_map_count_workspace_bytes", n, total)
    ws = arena.take(nbytes, label="count ws")
    call("spt_sparse_map_count", c32, gb, n, o_ptr, b_ptr, K, d, skeys, sorder, rowptr, record2, ws,
         nbytes)
    arena.check()
    assert record2.tolist() == [P, 0] and torch.equal(rowptr, kmap.rowptr)
    # fill
    nbr = fresh(arena, (P,), torch.int32, "nbr")
    off = fresh(arena, (P,), torch.int32, "off")
    row = fresh(arena, (P,), torch.int32, "row")
    call("spt_sparse_map_fill", c32, gb, n, o_ptr, b_ptr, K, d, skeys, sorder, rowptr, P, nbr, off, row)
    arena.check()
    assert torch.equal(nbr, kmap.nbr) and torch.equal(off, kmap.off) and torch.equal(row, kmap.row)
    # by offset
    perm = fresh(arena, (P,), torch.int32, "perm")
    optr = fresh(arena, (k3 + 1,), torch.int32, "optr")
    nbytes = query("spt_sparse_map_by_offset_workspace_bytes", P)
    ws = arena.take(nbytes, label="by-offset ws")
    call("spt_sparse_map_by_offset", off, P, k3, perm, optr, ws, nbytes)
    arena.check()
    assert torch.equal(perm, perm0) and torch.equal(optr, optr0)
    # forward, dX
    gx, gW, gbias, gg = put(arena, x, "x"), put(arena, W, "W"), put(arena, b, "bias"), put(arena, gout, "gout")
    out = fresh(arena, (n, co), torch.float32, "out")
    call("spt_sparse_conv_fwd_f32", gx, n, ci, gW, k3, co, gbias, rowptr, nbr, off, 0, out)
    arena.check()
    assert _bits(out, want[0])
    gWt = put(arena, W.transpose(1, 2).contiguous(), "Wt")
    dx = fresh(arena, (n, ci), torch.float32, "dX")
    call("spt_sparse_conv_fwd_f32", gg, n, co, gWt, k3, ci, None, rowptr, nbr, off, 1, dx)
    arena.check()
    assert _bits(dx, want[1])
    # dW, dbias
    dw = fresh(arena, (k3, ci, co), torch.float32, "dW")
    nbytes = query("spt_sparse_conv_dw_workspace_bytes", k3, ci, co)
    ws = arena.take(nbytes, label="dW ws")
    call("spt_sparse_conv_dw_f32", gx, gg, n, ci, co, k3, nbr, row, perm, optr, P, dw, ws, nbytes)
    arena.check()
    assert _bits(dw, want[2])
    db = fresh(arena, (co,), torch.float32, "dbias")
    nbytes = query("spt_sparse_conv_dbias_workspace_bytes", co)
    ws = arena.take(nbytes, label="dbias ws")
    call("spt_sparse_conv_dbias_f32", gg, n, co, db, ws, nbytes)
    arena.check()
    assert _bits(db, want[3])


def test_workspace_queries_and_refusals(dev):
    from superpoint_transformer_amd import _lib
    L = _lib.lib
    assert L.spt_sparse_map_count_workspace_bytes(0, 10) == 0
    assert L.spt_sparse_map_count_workspace_bytes(10, 64) == 0
    assert L.spt_sparse_map_count_workspace_bytes(5000, 40) > L.spt_sparse_map_count_workspace_bytes(5000, 20)
    assert L.spt_sparse_conv_dw_workspace_bytes(27, 65, 16) == 0
    assert L.spt_sparse_conv_dw_workspace_bytes(27, 32, 32) == 27 * 64 * 32 * 32 * 4
    assert L.spt_sparse_conv_dbias_workspace_bytes(0) == 0
    assert L.spt_sparse_conv_supported(7, 32) and L.spt_sparse_conv_supported(64, 64)
    assert not L.spt_sparse_conv_supported(65, 32) and not L.spt_sparse_conv_supported(7, 24)
    assert not L.spt_sparse_conv_supported(7, 80)
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    st = L.spt_sparse_map_count(t.data_ptr(), None, 4, None, None, 2, 1, None, None, None, None, None, 0,
                                _lib.stream_ptr(dev))
    assert st != 0


@pytest.mark.parametrize("ci,co,K,d", [(3, 32, 3, 1), (7, 16, 7, 1)])
def test_wrappers_on_exact_poisoned_scratch(ci, co, K, d, dev):
    from superpoint_transformer_amd import sparse as S
    coords, batch, x, W, b, gout = _case(150, ci, co, K, 7, dev)
    _, want = _plain(S, coords, batch, K, d, x, W, b, gout)
    for _ in range(2):
        arena = arena_for(dev)
        with poisoned_fresh_tensors(dev), exact_workspaces(arena):
            kmap, got = _plain(S, put(arena, coords, "coords"), put(arena, batch, "batch"), K, d,
                               put(arena, x, "x"), put(arena, W, "W"), put(arena, b, "b"),
                               put(arena, gout, "gout"))
        assert len(arena.sizes()) >= 9
        for name, g, w in zip(("out", "dX", "dW", "dbias"), got, want):
            assert _bits(g, w), name
