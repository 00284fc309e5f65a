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
