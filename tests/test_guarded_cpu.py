"""The guarded arena checks itself, on CPU tensors: what it must let pass, and what it must
report, with which offset and count (tests/guarded.py; its user is
tests/test_workspace_contract_gpu.py)."""
import pytest
import torch

import guarded
from guarded import GuardedArena, GuardError

CPU = torch.device("cpu")
G = 4096      # small guards: the checks read every guard byte


def _backing(arena, i=-1):
    label, back, start, nbytes = arena._slices[i]
    return back, start, nbytes


def test_slice_is_exact_and_aligned():
    a = GuardedArena(CPU, guard=G)
    for nbytes in (0, 1, 255, 256, 257, 4100):
        v = a.take(nbytes)
        assert v.dtype == torch.uint8 and v.numel() == nbytes
        assert v.data_ptr() % 256 == 0
        back, start, _ = _backing(a)
        assert start >= G and back.numel() - (start + nbytes) >= G
    t = a.take(4 * 15, torch.int32, (3, 5))
    assert t.dtype == torch.int32 and t.shape == (3, 5) and t.data_ptr() % 256 == 0
    u = a.like(torch.empty(7, 3, dtype=torch.float64))
    assert u.dtype == torch.float64 and u.shape == (7, 3)
    a.check()


def test_in_bounds_write_passes():
    a = GuardedArena(CPU, guard=G)
    v = a.take(1000, label="scratch")
    v.fill_(0)
    v[0] = 7
    v[-1] = 9
    t = a.take(8 * 33, torch.int64, (33,), label="out")
    t.fill_(-1)
    a.check()
    assert a.dirty() == []


def test_one_byte_past_the_end_is_reported_at_offset_0():
    a = GuardedArena(CPU, guard=G)
    a.take(512, label="other")
    a.take(1001, label="scan partials")          # an end that is no multiple of anything
    back, start, nbytes = _backing(a)
    back[start + nbytes] = 0
    assert a.dirty() == [("scan partials[1001 B]", "after", 0, 1)]
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert "scan partials" in msg and "offset 0 past its end" in msg and "1 guard byte" in msg
    assert "other" not in msg


def test_offset_and_count_of_a_longer_overrun():
    a = GuardedArena(CPU, guard=G)
    a.take(256, label="ws")
    back, start, nbytes = _backing(a)
    back[start + nbytes + 12:start + nbytes + 12 + 40] = 0
    assert a.dirty() == [("ws[256 B]", "after", 12, 40)]


def test_one_byte_before_the_start_is_reported():
    a = GuardedArena(CPU, guard=G)
    a.take(300, label="flags")
    back, start, _ = _backing(a)
    back[start - 1] = 1
    assert a.dirty() == [("flags[300 B]", "before", 0, 1)]
    with pytest.raises(GuardError) as e:
        a.check()
    assert "flags" in str(e.value) and "before its start" in str(e.value)


def test_writing_the_guard_byte_value_inside_is_not_an_error():
    a = GuardedArena(CPU, guard=G)
    v = a.take(64)
    v.fill_(guarded.GUARD_BYTE)
    a.check()


def test_exact_workspaces_patches_every_binding_and_restores():
    from superpoint_transformer_amd import data, neighbors, ops, segment
    holders = [ops, segment, neighbors, data]
    before = [m._workspace for m in holders]
    a = GuardedArena(CPU, guard=G)
    with guarded.exact_workspaces(a):
        for m in holders:
            assert m._workspace is ops._workspace          # one allocator everywhere
        assert ops._workspace is not before[0]
        w1 = segment._workspace(1234, CPU)
        w2 = neighbors._workspace(1234, CPU)
        assert w1.numel() == 1234 and w2.numel() == 1234
        assert w1.data_ptr() != w2.data_ptr()              # a fresh slice per call
        assert len(a) == 2
    assert [m._workspace for m in holders] == before


def test_exact_workspaces_checks_on_exit():
    a = GuardedArena(CPU, guard=G)
    with pytest.raises(GuardError) as e:
        with guarded.exact_workspaces(a):
            from superpoint_transformer_amd import ops
            ops._workspace(100, CPU)
            back, start, nbytes = _backing(a)
            back[start + nbytes + 3] = 0
    assert "_workspace#0" in str(e.value) and "offset 3" in str(e.value)


def test_exact_workspaces_refuses_another_device_of_the_same_kind():
    """An arena on one device must not let a request for another one of the same kind through to
    the grow-only buffer unnoticed (``cuda`` and ``cuda:0`` are the same device)."""
    from superpoint_transformer_amd import ops
    a = GuardedArena(CPU, guard=G)
    a.dev = torch.device("cuda", 1)                        # no allocation happens before the check
    with pytest.raises(GuardError) as e:
        with guarded.exact_workspaces(a):
            ops._workspace(64, torch.device("cuda", 0))
    assert "cuda:0" in str(e.value) and "cuda:1" in str(e.value)


# ---- the read-side probe: NaN guards, NaN scratch, NaN fresh tensors ---------------------------------
def _read(byte, dtype):
    return torch.full((8,), byte, dtype=torch.uint8).view(dtype)[0]


def test_how_each_dtype_reads_the_two_bytes():
    """0xA5 is a number nothing notices, 0xFF is NaN in every float format and -1 in the integers."""
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        assert bool(torch.isnan(_read(0xFF, dtype))), dtype
        assert bool(torch.isfinite(_read(0xA5, dtype))), dtype
    assert float(_read(0xA5, torch.float32)) == pytest.approx(-2.87e-16, rel=1e-2)
    assert float(_read(0xA5, torch.bfloat16)) == pytest.approx(-2.87e-16, rel=1e-2)
    assert float(_read(0xA5, torch.float64)) == pytest.approx(-2.5e-127, rel=1e-2)
    for dtype in (torch.int32, torch.int64):
        assert int(_read(0xFF, dtype)) == -1
        assert int(_read(0x00, dtype)) == 0
    # to a sum, a maximum or a product of ordinary numbers the 0xA5 value is zero
    one = torch.tensor(1.0)
    assert float(one + _read(0xA5, torch.float32)) == 1.0 and float(_read(0xA5, torch.float32) * 0) == 0.0
    assert bool(torch.isnan(_read(0xFF, torch.float32) * 0))


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (17, 3)), (torch.int64, (5,)), (torch.bfloat16, (7, 9)),
                                         (torch.float64, (1, 1)), (torch.uint8, (13,)), (torch.float32, (1,))])
def test_place_keeps_bits_alignment_and_the_flush_end(dtype, shape):
    a = GuardedArena(CPU, guard=G, guard_byte=0xFF)
    src = (torch.randn(shape) * 100).to(dtype)
    t = a.place(src, label="x")
    assert t.dtype == dtype and t.shape == src.shape and t.is_contiguous() and t._version == 0
    assert torch.equal(t.reshape(-1).view(torch.uint8), src.reshape(-1).view(torch.uint8))
    assert t.data_ptr() % 256 == 0
    back, start, nbytes = _backing(a)
    assert nbytes == src.numel() * src.element_size()
    assert back.data_ptr() + start == t.data_ptr()
    # the byte behind the last element and the byte in front of the first are guard bytes
    assert int(back[start + nbytes]) == 0xFF and int(back[start - 1]) == 0xFF
    a.check()


def test_placed_inputs_pass_the_wrappers_normalisation_without_a_copy():
    from superpoint_transformer_amd import ops
    a = GuardedArena(CPU, guard=G, guard_byte=0xFF)
    x = a.place(torch.randn(17, 5))
    i = a.place(torch.arange(17), guard_byte=0)
    assert ops._f32c(x).data_ptr() == x.data_ptr()
    assert ops._as_rows(x)[0].data_ptr() == x.data_ptr()
    assert x.contiguous().data_ptr() == x.data_ptr() and i.contiguous().data_ptr() == i.data_ptr()
    assert i.long().data_ptr() == i.data_ptr()


def test_each_slice_is_checked_against_its_own_byte():
    a = GuardedArena(CPU, guard=G, guard_byte=0xFF)
    a.take(100, label="nan-guarded")
    a.take(100, label="zero-guarded", guard_byte=0x00)
    a.place(torch.arange(9), guard_byte=0xA5, label="classic")
    for i, byte in enumerate((0xFF, 0x00, 0xA5)):
        back, start, nbytes = _backing(a, i)
        assert bool((back[:start] == byte).all()) and bool((back[start + nbytes:] == byte).all())
    a.check()
    # another slice's guard byte is a dirty byte here
    back, start, nbytes = _backing(a, 1)
    back[start + nbytes + 5] = 0xFF
    assert a.dirty() == [("zero-guarded[100 B]", "after", 5, 1)]
    back[start + nbytes + 5] = 0x00
    back, start, nbytes = _backing(a, 0)
    back[start - 2] = 0xA5
    assert a.dirty() == [("nan-guarded[100 B]", "before", 1, 1)]
    with pytest.raises(GuardError):
        a.check()


def test_defaults_are_the_old_arena():
    a = GuardedArena(CPU, guard=G)
    assert a.guard_byte == guarded.GUARD_BYTE == 0xA5 and a.fill_byte is None
    a.take(10)
    back, start, nbytes = _backing(a)
    assert bool((back[:start] == 0xA5).all()) and bool((back[start + nbytes:] == 0xA5).all())
    with pytest.raises(ValueError):
        GuardedArena(CPU, guard=G, guard_byte=256)


def test_fill_byte_reaches_workspaces_taken_through_exact_workspaces():
    from superpoint_transformer_amd import ops, segment
    a = GuardedArena(CPU, guard=G, guard_byte=0xFF, fill_byte=0xFF)
    with guarded.exact_workspaces(a):
        w = segment._workspace(4 * 33, CPU)
        assert bool((w == 0xFF).all()) and bool(torch.isnan(w.view(torch.float32)).all())
        assert bool((ops._workspace(8 * 5, CPU).view(torch.int64) == -1).all())
    t = a.take(8 * 6, torch.float64, (2, 3))
    assert bool(torch.isnan(t).all())
    assert GuardedArena(CPU, guard=G, fill_byte=0).take(16).tolist() == [0] * 16


def test_poisoned_fresh_tensors_poisons_floats_only_and_restores_every_name():
    names = [(o, n, getattr(o, n), n in vars(o)) for o, n in guarded.POISONED_FACTORIES]
    assert [n for _, n, _, _ in names] == ["empty", "empty_like", "empty_strided", "new_empty"]
    like = torch.zeros(3, 2)
    with guarded.poisoned_fresh_tensors(CPU):
        for t in (torch.empty(4, 5), torch.empty((4, 5), dtype=torch.bfloat16), torch.empty_like(like),
                  torch.empty_strided((3, 2), (2, 1)), like.new_empty((7,)), like.new_empty(2, 3, dtype=torch.float64),
                  torch.empty_like(like, dtype=torch.float16), torch.empty(2, device="cpu", dtype=torch.float32)):
            assert t.is_floating_point() and bool(torch.isnan(t).all()), t.dtype
        assert torch.empty(0, 3).shape == (0, 3)
        z = torch.zeros(5, dtype=torch.int64)
        for t in (torch.empty(5, dtype=torch.int64), torch.empty_like(z), z.new_empty(3),
                  torch.empty(4, dtype=torch.uint8), torch.empty(4, dtype=torch.bool)):
            assert not t.is_floating_point()                  # left alone (and no error filling them)
        assert torch.empty(3, dtype=torch.int32).dtype == torch.int32
    with guarded.poisoned_fresh_tensors(torch.device("cuda", 0)):
        assert torch.empty is not names[0][2]
        torch.empty(64).fill_(0)                              # another device's tensors: left alone, usable
    for o, n, real, own in names:
        assert getattr(o, n) is real and (n in vars(o)) == own, n
    with pytest.raises(RuntimeError, match="boom"):
        with guarded.poisoned_fresh_tensors(CPU):
            raise RuntimeError("boom")
    for o, n, real, own in names:
        assert getattr(o, n) is real and (n in vars(o)) == own, n


# ---- the probe has teeth: two stand-ins for the usual tail handling ---------------------------------------
TILE = 4


def _tile_sums(x, n, select):
    """A tiled kernel's tail handling in torch: whole tiles are loaded whatever ``n`` is, rows
    past the end are 'masked' - by a zero multiplier (``select=False``), or by a select after
    the load (``select=True``).  ``x`` is [n, c] inside a larger storage."""
    c = x.shape[1]
    tiles = -(-n // TILE)
    rows = torch.as_strided(x, (tiles * TILE, c), (c, 1))            # the unconditional load
    live = torch.arange(tiles * TILE) < n
    if select:
        rows = torch.where(live.view(-1, 1), rows, torch.zeros(()))
    else:
        rows = rows * live.view(-1, 1).to(x.dtype)
    return rows.view(tiles, TILE, c).sum(1)


def test_a_masked_read_past_the_end_shows_only_under_nan_guards():
    n, c = 7, 5                                                  # one row short of two tiles
    data = torch.randn(n + 1, c, generator=torch.Generator().manual_seed(5)) + 3
    plain = _tile_sums(data[:n], n, select=False)                # the row behind is another tensor's numbers
    right = torch.where((torch.arange(8) < n).view(-1, 1), data, torch.zeros(())).view(2, TILE, c).sum(1)
    assert torch.equal(plain, right)                             # ... and nothing shows: finite x 0
    old = GuardedArena(CPU, guard=G)                             # 0xA5 guards
    got = _tile_sums(old.place(data[:n]), n, select=False)
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    nan = GuardedArena(CPU, guard=G, guard_byte=0xFF)
    got = _tile_sums(nan.place(data[:n]), n, select=False)
    assert bool(torch.isnan(got[1]).all()) and torch.equal(got[0], plain[0])
    # the repair (select after the load) reads the same bytes and is clean under both
    for arena in (old, nan):
        got = _tile_sums(arena.place(data[:n]), n, select=True)
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
        arena.check()


def _sum_by_blocks(x, ws, blocks):
    """A two-pass reduction: each block with rows writes its partial sum to the table in ``ws``,
    the second pass sums all ``blocks`` rows of the table - also those of blocks that had no
    rows and wrote nothing."""
    c = x.shape[1]
    table = ws.view(torch.float32)[:blocks * c].view(blocks, c)
    for b, rows in enumerate(x.chunk(blocks)):                   # fewer chunks than blocks: rows run out
        table[b] = rows.sum(0)
    return table.sum(0)


def test_an_unwritten_partial_shows_only_under_nan_scratch():
    blocks, c = 4, 6
    x = torch.rand(3, c, generator=torch.Generator().manual_seed(6)) + 1      # 3 rows: block 3 has none
    right = torch.cat((x, torch.zeros(1, c))).sum(0)
    old = GuardedArena(CPU, guard=G, fill_byte=0xA5)
    got = _sum_by_blocks(x, old.take(4 * blocks * c), blocks)
    assert torch.equal(got.view(torch.int32), right.view(torch.int32))       # -2.87e-16 is nothing to a sum
    nan = GuardedArena(CPU, guard=G, guard_byte=0xFF, fill_byte=0xFF)
    got = _sum_by_blocks(x, nan.take(4 * blocks * c), blocks)
    assert bool(torch.isnan(got).all())
    # with every partial written the poisoned scratch changes nothing
    x4 = torch.cat((x, torch.zeros(1, c)))
    got = _sum_by_blocks(x4, nan.take(4 * blocks * c), blocks)
    assert torch.equal(got.view(torch.int32), right.view(torch.int32))
    old.check()
    nan.check()
