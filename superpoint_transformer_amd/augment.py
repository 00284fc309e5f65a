"""Augmentation passes of the per-batch training chain (csrc/augment.hip): jitter, column and
row dropout, rotation / scale / flip of positions, normals and 7-column edge attributes, colour
auto-contrast and drop.  One launch per tensor, every parameter explicit, no host read.

Random stream (shared with ``segment.sparse_sample``): ``r = rand32(seed, counter)``, the
splitmix64 finaliser.  The counter of an element is its logical index ``row * n_cols + col``, the
counter of a row decision is ``row``; nothing depends on strides, alignment or grid size.

  * decisions: ``u = (r >> 8) * 2**-24`` in [0, 1), taken when ``u < float32(p)``, like
    ``torch.rand(...) < p``;
  * noise: ``u = ((r >> 8) + 0.5) * 2**-24`` in (0, 1) and the construction of
    ``torch.nn.init.trunc_normal_``: ``clamp(sigma * sqrt(2) * erfinv(lo + u * (hi - lo)),
    -trunc, trunc)`` with ``lo = 2 Phi(-trunc / sigma) - 1``, ``hi = 2 Phi(trunc / sigma) - 1``.
    ``trunc <= 0`` (where the reference calls ``randn_like``): ``lo = -1``, ``hi = 1``, no clamp.
    There is ONE generator, 24 bits per draw, so the untruncated tail ends at
    ``sqrt(2) * erfinv(1 - 2**-24) = 5.42 sigma``; the noise is always finite.

CUDA tensors run the kernels; a missing kernel is an error.  CPU tensors take a torch composition
of the same formulas over a torch restatement of ``rand32`` so that the transform classes can be
tested without a GPU: decisions are bit-identical to the kernels', the noise (f64 ``erfinv``
rounded to f32) is not guaranteed to be.
"""
import ctypes
import math

import torch

from . import _lib
from .segment import _draw_seed

__all__ = ["rand32", "unit", "noise", "noise_bounds", "features_", "jitter_", "dropout_",
           "geometry_", "color_range", "color_", "column_mask", "LAUNCHES", "POS", "NORMAL", "EDGE7"]

POS, NORMAL, EDGE7 = 0, 1, 2
_M64 = (1 << 64) - 1

# kernel launches made by this module since import (tools/augment_bench.py reads it)
LAUNCHES = {"kernels": 0, "fills": 0}


# ---------------------------------------------------------------------------
# the generator, restated in torch (int64 arithmetic wraps; shifts are arithmetic: mask after)
# ---------------------------------------------------------------------------
def _s64(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def rand32(seed, counters):
    """``rand32(seed, counter)`` of csrc/rng.hpp for an int64 tensor of counters: int64 values
    in [0, 2**32)."""
    i = counters.to(torch.int64)
    z = (i + 1) * _s64(0x9E3779B97F4A7C15) + _s64(int(seed))
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _s64(0x94D049BB133111EB)
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return (z >> 32) & 0xFFFFFFFF


def unit(seed, counters):
    """Decision uniforms in [0, 1): f32, exact."""
    return (rand32(seed, counters) >> 8).to(torch.float32) * (2.0 ** -24)


def noise_bounds(sigma, trunc):
    """(lo, hi) of the truncated normal in f64: ``2 Phi(-+trunc / sigma) - 1 = erf(-+trunc /
    (sigma sqrt 2))``; (-1, 1) for ``trunc <= 0``."""
    if trunc <= 0:
        return -1.0, 1.0
    h = math.erf(float(trunc) / float(sigma) / math.sqrt(2.0))
    return -h, h


def noise(seed, counters, sigma, trunc):
    """The noise of the given counters in f64 (the CPU route rounds it to f32)."""
    lo, hi = noise_bounds(sigma, trunc)
    u = ((rand32(seed, counters) >> 8).to(torch.float64) + 0.5) * (2.0 ** -24)
    z = float(sigma) * math.sqrt(2.0) * torch.special.erfinv(lo + u * (hi - lo))
    if trunc > 0:
        z = z.clamp(-float(trunc), float(trunc))
    return z


def column_mask(columns):
    """64-bit mask of an iterable of column indices."""
    m = 0
    for c in columns:
        c = int(c)
        if not 0 <= c < 64:
            raise ValueError(f"column {c} outside 0..63")
        m |= 1 << c
    return m


# ---------------------------------------------------------------------------
def _block(t, name="x", cols=None):
    """(n, n_cols, row stride in elements) of a [n] or [n, c] f32 tensor with unit column
    stride: a tensor of its own or a column slice of a wider table."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if t.dim() == 1:
        n, c, ld = t.shape[0], 1, (t.stride(0) if t.shape[0] > 1 else 1)
    elif t.dim() == 2:
        n, c = t.shape
        if c > 1 and t.stride(1) != 1:
            raise ValueError(f"{name}: columns must be adjacent in memory")
        ld = t.stride(0) if n > 1 else max(c, 1)
    else:
        raise ValueError(f"{name} must be [n] or [n, c], got {tuple(t.shape)}")
    if cols is not None and c != cols:
        raise ValueError(f"{name} must have {cols} columns, got {c}")
    if c < 1 or (n > 1 and ld < c):
        raise ValueError(f"{name}: rows overlap or no columns")
    return n, c, ld


def _out_like(x, out):
    if out is None:
        return x
    if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise ValueError("out must match x in shape, dtype and device")
    return out


def _noise_args(jitter):
    """jitter = None | (sigma, trunc, seed) -> (on, seed, sigma, trunc, lo, hi)."""
    if jitter is None:
        return False, 0, 0.0, 0.0, -1.0, 1.0
    sigma, trunc, seed = jitter
    if not sigma > 0:
        raise ValueError("jitter needs sigma > 0")
    seed = _draw_seed() if seed is None else int(seed)
    lo, hi = noise_bounds(sigma, trunc)
    return True, seed & _M64, float(sigma), float(trunc), lo, hi


def _counters(n, c, dev):
    return torch.arange(n * c, dtype=torch.int64, device=dev).view(n, c)


def _view2(t):
    return t.unsqueeze(1) if t.dim() == 1 else t


def _launch(fn, name, *args):
    st = fn(*args)
    _lib.check(st, name)
    LAUNCHES["kernels"] += 1


# ---------------------------------------------------------------------------
def features_(x, jitter=None, col_mask=None, p_rows=None, seed_rows=None, out=None):
    """In one pass, in this order: ``x += noise`` (``jitter = (sigma, trunc, seed)``), zero the
    columns of ``col_mask`` (an int, see ``column_mask``), zero the rows ``i`` with
    ``u(seed_rows, i) < p_rows``.  Writes ``out`` (default: ``x`` itself) and returns it."""
    n, c, ld = _block(x)
    out = _out_like(x, out)
    _, _, ld_out = _block(out, "out")
    on, seed, sigma, trunc, lo, hi = _noise_args(jitter)
    flags = (1 if on else 0) | (2 if col_mask is not None else 0) | (4 if p_rows is not None else 0)
    if flags == 0:
        raise ValueError("nothing to do: give jitter, col_mask or p_rows")
    mask = int(col_mask or 0)
    if col_mask is not None and (c > 64 or mask >> c):
        raise ValueError("col_mask addresses columns the tensor does not have (n_cols <= 64)")
    if p_rows is not None and seed_rows is None:
        seed_rows = _draw_seed()
    seed_rows = int(seed_rows or 0) & _M64
    p = float(p_rows or 0.0)
    if n == 0:
        return out
    if x.is_cuda:
        with torch.cuda.device(x.device):
            _launch(_lib.lib.spt_augment_features_f32, "spt_augment_features_f32", _lib.ptr(x),
                    _lib.ptr(out), n, c, ld, ld_out, flags, seed, sigma, trunc, lo, hi, mask,
                    seed_rows, p, _lib.stream_ptr(x.device))
        return out
    v = _view2(x)
    if on:
        v = v + noise(seed, _counters(n, c, x.device), sigma, trunc).to(torch.float32)
    else:
        v = v.clone()
    if col_mask is not None:
        v[:, [j for j in range(c) if (mask >> j) & 1]] = 0.0
    if p_rows is not None:
        drop = unit(seed_rows, torch.arange(n)) < torch.tensor(p, dtype=torch.float32)
        v[drop] = 0.0
    _view2(out).copy_(v)
    return out


def jitter_(x, sigma, trunc, seed=None, out=None):
    """``x += noise`` (NAGJitterKey on one tensor)."""
    return features_(x, jitter=(sigma, trunc, seed), out=out)


def dropout_(x, col_mask=None, p_rows=None, seed_rows=None, out=None):
    """Zero the columns of ``col_mask`` and / or the rows drawn with ``p_rows``."""
    return features_(x, col_mask=col_mask, p_rows=p_rows, seed_rows=seed_rows, out=out)


def _f32_list(v, k, name):
    t = torch.as_tensor(v, dtype=torch.float32)
    if t.is_cuda:
        raise ValueError(f"{name} must live on the host: it is passed by value")
    t = t.reshape(-1)
    if t.numel() != k:
        raise ValueError(f"{name} must hold {k} values")
    return [float(a) for a in t]


def geometry_(x, mode, jitter=None, R=None, scale=None, flip_axis=None, out=None):
    """One pass over ``pos`` (``POS``), a normal (``NORMAL``) or a 7-column ``edge_attr``
    (``EDGE7``); every step is optional, the order is fixed:

      POS     jitter, ``v @ R.T``, ``v * scale``, negate column ``flip_axis``
      NORMAL  rotate, negate rows with z < 0, scale and ``v / max(||v||, 1e-12)``, flip, negate
              rows with z < 0
      EDGE7   columns 0:3 rotate, scale, flip; columns 3:7 times ``||scale||_2`` (with the scale)

    ``R`` (3 x 3) and ``scale`` (3) are HOST values.  The fused call gives the bits of the steps
    made one by one."""
    w = 7 if mode == EDGE7 else 3
    if mode not in (POS, NORMAL, EDGE7):
        raise ValueError("mode must be POS, NORMAL or EDGE7")
    if x.dim() != 2 or x.shape[1] != w:
        raise ValueError(f"expected {w} columns, got {tuple(x.shape)}")
    n, _, ld = _block(x)
    out = _out_like(x, out)
    _, _, ld_out = _block(out, "out")
    if jitter is not None and mode != POS:
        raise ValueError("jitter is a step of the POS mode")
    on, seed, sigma, trunc, lo, hi = _noise_args(jitter)
    flags = (1 if on else 0) | (2 if R is not None else 0) | (4 if scale is not None else 0) \
        | (8 if flip_axis is not None else 0)
    if flags == 0:
        raise ValueError("nothing to do: give jitter, R, scale or flip_axis")
    r9 = _f32_list(R, 9, "R") if R is not None else [0.0] * 9
    s3 = _f32_list(scale, 3, "scale") if scale is not None else [1.0] * 3
    # ||scale||_2 as Tensor.norm gives it in f32
    snorm = float(torch.tensor(s3, dtype=torch.float32).norm())
    axis = int(flip_axis) if flip_axis is not None else 0
    if not 0 <= axis <= 2:
        raise ValueError("flip_axis must be 0, 1 or 2")
    if n == 0:
        return out
    if x.is_cuda:
        with torch.cuda.device(x.device):
            _launch(_lib.lib.spt_augment_geometry_f32, "spt_augment_geometry_f32", _lib.ptr(x),
                    _lib.ptr(out), n, ld, ld_out, mode, flags, seed, sigma, trunc, lo, hi,
                    (ctypes.c_float * 9)(*r9), (ctypes.c_float * 3)(*s3), snorm, axis,
                    _lib.stream_ptr(x.device))
        return out
    v = x.clone()
    a = v[:, :3]

    def up(t):
        neg = t[:, 2] < 0
        t[neg] = -t[neg]

    if on:
        a += noise(seed, _counters(n, 3, x.device), sigma, trunc).to(torch.float32)
    if R is not None:
        Rm = torch.tensor(r9, dtype=torch.float32).view(3, 3)
        x0, y0, z0 = a[:, 0].clone(), a[:, 1].clone(), a[:, 2].clone()
        for i in range(3):
            a[:, i] = Rm[i, 0] * x0 + Rm[i, 1] * y0 + Rm[i, 2] * z0
        if mode == NORMAL:
            up(a)
    if scale is not None:
        a *= torch.tensor(s3, dtype=torch.float32)
        if mode == NORMAL:
            a /= (a * a).sum(1, keepdim=True).sqrt().clamp_min(1e-12)
        if mode == EDGE7:
            v[:, 3:] *= torch.tensor(snorm, dtype=torch.float32)
    if flip_axis is not None:
        a[:, axis] = -a[:, axis]
        if mode == NORMAL:
            up(a)
    out.copy_(v)
    return out


def color_range(color, jitter=None, out=None):
    """``[min of columns 0..2, max of columns 0..2]`` of the (jittered) colours as 6 floats on
    the colours' device, without storing the jittered colours."""
    n, _, ld = _block(color, "color", cols=3)
    if out is None:
        out = torch.empty(6, dtype=torch.float32, device=color.device)
    on, seed, sigma, trunc, lo, hi = _noise_args(jitter)
    if n == 0:
        return out
    if color.is_cuda:
        with torch.cuda.device(color.device):
            _launch(_lib.lib.spt_augment_color_range_f32, "spt_augment_color_range_f32",
                    _lib.ptr(color), n, ld, int(on), seed, sigma, trunc, lo, hi, _lib.ptr(out),
                    _lib.stream_ptr(color.device))
        LAUNCHES["fills"] += 2
        return out
    v = color
    if on:
        v = v + noise(seed, _counters(n, 3, color.device), sigma, trunc).to(torch.float32)
    out[:3] = v.min(0).values
    out[3:] = v.max(0).values
    return out


def color_(color, jitter=None, contrast=None, drop=False, out=None, range6=None):
    """In one pass: jitter (``(sigma, trunc, seed)``), auto-contrast (``contrast = blend`` or
    ``(blend, one_minus_blend)``: ``(1 - b) c + b (c - lo) / (hi - lo)`` with the per-column
    range of the JITTERED colours, IEEE division), drop (``c * 0``).  With a contrast the range
    takes a launch of its own (``color_range``) unless ``range6`` is given."""
    n, _, ld = _block(color, "color", cols=3)
    out = _out_like(color, out)
    _, _, ld_out = _block(out, "out")
    if jitter is not None and jitter[2] is None:
        jitter = (jitter[0], jitter[1], _draw_seed())
    on, seed, sigma, trunc, lo, hi = _noise_args(jitter)
    flags = (1 if on else 0) | (2 if contrast is not None else 0) | (4 if drop else 0)
    if flags == 0:
        raise ValueError("nothing to do: give jitter, contrast or drop")
    b, omb = 0.0, 1.0
    if contrast is not None:
        if isinstance(contrast, (tuple, list)):
            b, omb = float(contrast[0]), float(contrast[1])
        else:
            b = float(contrast)
            omb = 1.0 - b
    if n == 0:
        return out
    if contrast is not None and range6 is None:
        range6 = color_range(color, jitter)
    if color.is_cuda:
        with torch.cuda.device(color.device):
            _launch(_lib.lib.spt_augment_color_f32, "spt_augment_color_f32", _lib.ptr(color),
                    _lib.ptr(out), n, ld, ld_out, flags, seed, sigma, trunc, lo, hi,
                    _lib.ptr(range6), b, omb, _lib.stream_ptr(color.device))
        return out
    v = color
    if on:
        v = v + noise(seed, _counters(n, 3, color.device), sigma, trunc).to(torch.float32)
    if contrast is not None:
        lo3, hi3 = range6[:3].view(1, 3), range6[3:].view(1, 3)
        f = (v - lo3) / (hi3 - lo3)
        v = torch.tensor(omb, dtype=torch.float32) * v + torch.tensor(b, dtype=torch.float32) * f
    if drop:
        v = v * 0.0
    out.copy_(v)
    return out
