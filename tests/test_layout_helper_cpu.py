"""``_lib.dense``: the one normaliser between a PyTorch tensor's layout and the kernels' contract
(row-major, contiguous, the entry's element type, an aligned base).  CPU tensors, no device: the
helper only reads ``dtype`` / ``is_contiguous()`` / ``data_ptr()``, so the same variants the GPU
layout suite sends through the wrappers are checked here for what comes back:

  * a dense, aligned tensor of the right type is returned AS IS (the same object: no copy on the
    hot path);
  * every other layout comes back as a dense aligned copy with the same values, and the source -
    the skipped elements of its parent buffer included - is left untouched.
"""
import pytest
import torch

from superpoint_transformer_amd import _lib

N, C = 17, 6


def _aligned_flat(numel, dtype, lead):
    """A flat buffer whose element ``lead`` sits on a 16-byte boundary (torch's CPU allocator
    aligns to 64 bytes; the assertion keeps the test honest should that ever change)."""
    flat = torch.zeros(numel + lead + 8, dtype=dtype)
    assert flat.data_ptr() % 16 == 0
    return flat


def _values(n=N, c=C, dtype=torch.float32):
    return (torch.arange(n * c, dtype=torch.float64).reshape(n, c) * 0.37 - 5).to(dtype)


def _views(dtype=torch.float32):
    """name -> (view, parent buffer) of the same [N, C] values in each layout of the suite."""
    v = _values(dtype=dtype)
    out = {}
    wide = torch.full((N, C + 7), float("nan"), dtype=dtype)
    wide[:, 3:3 + C] = v
    out["colslice"] = (wide[:, 3:3 + C], wide)
    big = torch.full((2 * N, C), float("nan"), dtype=dtype)
    big[::2] = v
    out["rowstride"] = (big[::2], big)
    xt = v.t().contiguous()
    out["transposed"] = (xt.t(), xt)
    for name, lead in (("off4", 1), ("off8", 2)):
        flat = _aligned_flat(N * C, dtype, lead)
        flat.fill_(float("nan"))
        flat[lead:lead + N * C] = v.reshape(-1)
        out[name] = (flat[lead:lead + N * C].view(N, C), flat)
    return v, out


def test_dense_aligned_tensor_is_returned_as_is():
    x = _values()
    assert x.data_ptr() % 16 == 0
    assert _lib.dense(x) is x
    assert _lib.dense(x, torch.float32) is x
    assert _lib.dense(x, torch.float32, 16) is x
    i = torch.arange(N)
    assert _lib.dense(i, torch.int64, 8) is i
    assert _lib.dense(None) is None and _lib.dense(None, torch.float32) is None
    # one row of a wider table is dense whatever its row stride says
    row = torch.zeros(4, 8)[0:1]
    assert _lib.dense(row) is row
    # no rows at all: nothing to read, nothing to copy
    e = torch.empty(0, C)
    assert _lib.dense(e, torch.float32) is e


@pytest.mark.parametrize("name", ["colslice", "rowstride", "transposed", "off4", "off8"])
def test_views_become_dense_aligned_copies(name):
    v, views = _views()
    view, parent = views[name]
    assert torch.equal(view, v)
    if name in ("off4", "off8"):
        assert view.is_contiguous() and view.data_ptr() % 16 == (4 if name == "off4" else 8)
    else:
        assert not view.is_contiguous()
    before = parent.clone()
    d = _lib.dense(view, torch.float32)
    assert d is not view and d.data_ptr() != view.data_ptr()
    assert d.is_contiguous() and d.data_ptr() % 16 == 0
    assert d.dtype == torch.float32 and d.shape == view.shape
    assert torch.equal(d, v)
    # the source and the elements skipped around it are as they were (NaN compares by bits)
    assert torch.equal(parent.view(torch.int32), before.view(torch.int32))
    # a second pass has nothing left to do
    assert _lib.dense(d, torch.float32) is d


def test_expanded_rows():
    row = _values(1, C)
    x = row.expand(N, C)
    assert x.stride(0) == 0
    d = _lib.dense(x, torch.float32)
    assert d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, row.repeat(N, 1))
    s = torch.tensor(2.5).expand(N, C)                  # what out.sum().backward() hands over
    d = _lib.dense(s, torch.float32)
    assert d.is_contiguous() and d.shape == (N, C) and bool((d == 2.5).all())


@pytest.mark.parametrize("src,dst", [(torch.float64, torch.float32), (torch.bfloat16, torch.float32),
                                     (torch.int32, torch.int64), (torch.bool, torch.uint8)])
def test_dtype_cast(src, dst):
    if src.is_floating_point:
        x = _values(dtype=src)
    elif src == torch.bool:
        x = (torch.arange(N * C).reshape(N, C) % 3 == 0)
    else:
        x = torch.arange(N * C, dtype=src).reshape(N, C)
    d = _lib.dense(x, dst, 8)
    assert d.dtype == dst and d.is_contiguous() and d.data_ptr() % 8 == 0
    assert torch.equal(d, x.to(dst))
    # cast and layout together: a strided view of another type
    big = torch.zeros((2 * N, C), dtype=src)
    big[::2] = x
    d2 = _lib.dense(big[::2], dst, 8)
    assert d2.dtype == dst and d2.is_contiguous() and torch.equal(d2, x.to(dst))


def test_index_views():
    """The index layouts of the suite: ``pairs.t()`` ([2, E] over [E, 2] storage), a column of a
    table, every other row, a flat-buffer view that starts 8 bytes into a 16-byte line (dense and
    8-byte aligned: int64 indices are read one element at a time, so it passes as is)."""
    E = 13
    pairs = torch.arange(2 * E).reshape(E, 2)
    ei = pairs.t()
    d = _lib.dense(ei, torch.int64, 8)
    assert d is not ei and d.is_contiguous() and torch.equal(d, pairs.t().contiguous())
    table = torch.arange(3 * N).reshape(N, 3)
    d = _lib.dense(table[:, 1], torch.int64, 8)
    assert d.is_contiguous() and torch.equal(d, table[:, 1].clone())
    big = torch.arange(2 * N)
    assert torch.equal(_lib.dense(big[::2], torch.int64, 8), torch.arange(0, 2 * N, 2))
    flat = _aligned_flat(N, torch.int64, 1)
    v = flat[1:1 + N]
    assert v.data_ptr() % 16 == 8
    assert _lib.dense(v, torch.int64, 8) is v
    c = _lib.dense(v, torch.int64, 16)                  # an entry that did ask for 16 bytes
    assert c is not v and c.data_ptr() % 16 == 0 and torch.equal(c, v)


def test_gradient_views_of_autograd():
    """The two gradient layouts ordinary autograd produces: the stride-0 gradient of ``sum()`` and
    the column-slice gradient ``gout[:, 4:]`` whose base sits 16 bytes into a row."""
    gout = _values(N, 4 + C)
    g = gout[:, 4:]
    assert not g.is_contiguous()
    d = _lib.dense(g, torch.float32)
    assert d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, g)
