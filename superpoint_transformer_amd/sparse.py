"""Stride-1 sparse 3D convolution over integer voxel coordinates (what ``torchsparse.nn.Conv3d``
does for ``src/nn/sparse.py``) on the kernels of ``csrc/sparse_conv.hip``.  DESIGN 7.23 is the
specification; in short, for N active voxels, odd K, r = K // 2, dilation d:

    out[i] = bias + sum over o = 0 .. K^3 - 1, ascending, of  x[j(i, o)] @ W[o]
    j(i, o) = the voxel of the same batch item at coords[i] + d * delta(o), if there is one
    delta(o) = (dx, dy, dz),  o = ((dz + r) * K + (dy + r)) * K + (dx + r)        (x fastest)
    W: [K^3, C_in, C_out];  K = 1: [C_in, C_out]

``kernel_offsets`` is the ONE place that fixes the offset order.  It is what torchsparse 2.1 is
believed to use for an odd kernel volume and is unverified: a checkpoint trained
under the mirrored convention loads as ``W.flip(0)``, one under another axis order as a fixed
permutation of axis 0 - at load time, with no kernel touched.

``build_kernel_map`` -> ``KernelMap``: the pairs as CSR by output voxel (``rowptr`` [N + 1],
and per pair ``nbr``, ``off`` ascending inside a voxel, ``row``), all int32.  Host reads on the
device, two per map: the bounds record (sizes the padded key, refuses one beyond 63 bits) and
the (pairs, duplicates) record (sizes the pair arrays, refuses duplicates and 2^31 pairs or
more); float coords cost a third (the integrality check).  ``sparse_conv3d`` on a built map
reads nothing back - forward and backward fit a captured step, once ``prepare_backward`` (or a
first backward) has listed the pairs by offset for dW.

CPU tensors, and on the device the shapes the kernel does not take (C_in > 64, C_out no multiple
of 16 or > 64, non-f32), run a torch composition of the same rules: map from sort +
``searchsorted``; per offset, ascending, gather -> matmul -> ``index_add_`` (it reads the
per-offset counts back to the host)."""
import contextlib

import torch

from . import _lib

__all__ = ["KernelMap", "kernel_offsets", "build_kernel_map", "sparse_conv3d", "kernel_supported",
           "composition_only", "MAX_KEY_BITS", "MAX_KERNEL_SIZE"]

MAX_KEY_BITS = 63
MAX_KERNEL_SIZE = 15
_INT32_MAX = (1 << 31) - 1
_FORCE_COMPOSITION = False


@contextlib.contextmanager
def composition_only(on=True):
    """Inside the block ``sparse_conv3d`` takes the torch composition on every device (what the
    model tests compare the kernels with)."""
    global _FORCE_COMPOSITION
    prev, _FORCE_COMPOSITION = _FORCE_COMPOSITION, bool(on)
    try:
        yield
    finally:
        _FORCE_COMPOSITION = prev


def _kernel_size(kernel_size):
    if isinstance(kernel_size, (tuple, list)) or hasattr(kernel_size, "__len__"):
        ks = [int(k) for k in kernel_size]
        if len(ks) != 3 or len(set(ks)) != 1:
            raise ValueError(f"kernel_size must be one int (or three equal ones), got {kernel_size}")
        kernel_size = ks[0]
    k = int(kernel_size)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"even kernel sizes are not built (odd K >= 1 only), got {k}")
    if k > MAX_KERNEL_SIZE:
        raise ValueError(f"kernel_size beyond {MAX_KERNEL_SIZE} is not built, got {k}")
    return k


def _dilation(dilation):
    if isinstance(dilation, (tuple, list)):
        ds = [int(v) for v in dilation]
        if len(ds) != 3 or len(set(ds)) != 1:
            raise ValueError(f"dilation must be one int (or three equal ones), got {dilation}")
        dilation = ds[0]
    d = int(dilation)
    if d < 1 or d > (1 << 20):
        raise ValueError(f"dilation must be in 1 .. 2^20, got {d}")
    return d


def check_stride(stride=1, transposed=False):
    """Raises for what is not built: strided and transposed sparse convolutions."""
    s = list(stride) if isinstance(stride, (tuple, list)) else [stride]
    if any(int(v) != 1 for v in s):
        raise NotImplementedError(f"strided sparse convolutions are not built (stride 1 only), got "
                                  f"stride={stride}")
    if transposed:
        raise NotImplementedError("transposed sparse convolutions are not built")


def kernel_offsets(kernel_size, dilation=1):
    """``[K^3, 3]`` int64: row o = d * (dx, dy, dz) with o = ((dz + r) K + (dy + r)) K + (dx + r)."""
    k, d = _kernel_size(kernel_size), _dilation(dilation)
    r = k // 2
    ax = torch.arange(-r, r + 1, dtype=torch.int64)
    dz, dy, dx = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.stack([dx.reshape(-1), dy.reshape(-1), dz.reshape(-1)], dim=1) * d


class KernelMap:
    """The pairs of a stride-1 sparse convolution, CSR by output voxel: voxel i owns the pairs
    [rowptr[i], rowptr[i + 1]) with ``off`` ascending; ``nbr`` is the neighbour, ``row`` is i.
    ``by_offset()`` adds the same pairs stably sorted by offset (``perm`` [P], ``optr`` [K^3 + 1])
    for dW and for the torch composition."""

    def __init__(self, n, kernel_size, dilation, rowptr, nbr, off, row):
        self.n, self.kernel_size, self.dilation = int(n), int(kernel_size), int(dilation)
        self.k3 = self.kernel_size ** 3
        self.rowptr, self.nbr, self.off, self.row = rowptr, nbr, off, row
        self.num_pairs = int(nbr.numel())
        self._by_offset = None
        self._by_offset_torch = None

    @property
    def device(self):
        return self.rowptr.device

    @property
    def pairs_per_voxel(self):
        return self.num_pairs / max(self.n, 1)

    def by_offset(self):
        """(perm int32 [P], optr int32 [K^3 + 1]) on the device route, built once; no host read."""
        if self._by_offset is None:
            if not self.rowptr.is_cuda:
                perm, optr = self.by_offset_torch()
                self._by_offset = (perm.int(), optr.int())
                return self._by_offset
            from .ops import _workspace
            dev = self.device
            perm = torch.empty(self.num_pairs, dtype=torch.int32, device=dev)
            optr = torch.empty(self.k3 + 1, dtype=torch.int32, device=dev)
            L = _lib.lib
            nbytes = L.spt_sparse_map_by_offset_workspace_bytes(self.num_pairs)
            ws = _workspace(nbytes, dev)
            with torch.cuda.device(dev):
                st = L.spt_sparse_map_by_offset(_lib.ptr(self.off), self.num_pairs, self.k3,
                                                _lib.ptr(perm), _lib.ptr(optr), _lib.ptr(ws), nbytes,
                                                _lib.stream_ptr(dev))
            _lib.check(st, "spt_sparse_map_by_offset")
            self._by_offset = (perm, optr)
        return self._by_offset

    prepare_backward = by_offset

    def by_offset_torch(self):
        """(perm int64 [P], optr int64 [K^3 + 1]) by torch's stable sort."""
        if self._by_offset_torch is None:
            off = self.off.long()
            perm = torch.sort(off, stable=True).indices
            counts = torch.bincount(off, minlength=self.k3)
            optr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
            self._by_offset_torch = (perm, optr)
        return self._by_offset_torch


def _check_coords(coords, batch):
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be [N, 3] (x, y, z), got {tuple(coords.shape)}")
    n = coords.shape[0]
    if n == 0:
        raise ValueError("no active voxel")
    if n > _INT32_MAX:
        raise ValueError("2^31 voxels or more")
    if coords.dtype == torch.bool or coords.is_complex():
        raise ValueError("coords must be integers")
    coords = coords.detach()
    if coords.is_floating_point():
        # QuantizePointCoordinates hands floats that hold integers; anything else is refused
        if not bool(((coords == coords.round()) & torch.isfinite(coords)).all()):      # host read
            raise ValueError("non-integer coords: a sparse convolution runs on integer voxel "
                             "coordinates (quantise the positions first)")
    if batch is not None:
        if batch.dim() != 1 or batch.numel() != n:
            raise ValueError("batch must hold one index per voxel")
        if batch.is_floating_point():
            raise ValueError("batch must be an integer tensor")
        batch = batch.detach()
    return n, coords, batch


def _key_layout(mins, maxs, pad):
    """Padded origin and field widths (x, y, z, batch); raises beyond 63 bits."""
    origin = [int(mins[0]) - pad, int(mins[1]) - pad, int(mins[2]) - pad, int(mins[3])]
    ext = [int(maxs[a]) - int(mins[a]) + (2 * pad if a < 3 else 0) for a in range(4)]
    bits = [e.bit_length() for e in ext]
    total = sum(bits)
    if total > MAX_KEY_BITS:
        raise ValueError(
            f"the padded voxel key needs {total} bits (x {bits[0]}, y {bits[1]}, z {bits[2]}, batch "
            f"{bits[3]}) for coordinates {list(zip(mins, maxs))} padded by {pad}: more than "
            f"{MAX_KEY_BITS}; a far outlier is the likely cause")
    return origin, bits, total


def _refuse(dups, pairs):
    if dups:
        raise ValueError(f"{dups} duplicate (batch, coords) row(s): a sparse tensor holds each voxel "
                         "once (voxelise first)")
    if pairs > _INT32_MAX:
        raise ValueError(f"the kernel map has {pairs} pairs: 2^31 or more")


def _map_torch(coords, batch, n, k, d):
    c = coords.long()
    cols = [c[:, 0], c[:, 1], c[:, 2], batch.long() if batch is not None else c.new_zeros(n)]
    mins = [int(v.min()) for v in cols]
    maxs = [int(v.max()) for v in cols]
    if max(abs(v) for v in mins[:3] + maxs[:3]) > _INT32_MAX - 1:
        raise ValueError("a coordinate does not fit 32 bits")
    r = k // 2
    origin, bits, _ = _key_layout(mins, maxs, r * d)
    key = torch.zeros(n, dtype=torch.int64, device=c.device)
    shifts, shift = [], 0
    for v, lo, b in zip(cols, origin, bits):
        key |= (v - lo) << shift
        shifts.append(shift)
        shift += b
    skeys, order = torch.sort(key)
    dups = int((skeys[1:] == skeys[:-1]).sum())
    _refuse(dups, 0)
    rows, nbrs, offs = [], [], []
    arange = torch.arange(n, device=c.device)
    for o, (dx, dy, dz) in enumerate(kernel_offsets(k, d).tolist()):
        target = key + (dx << shifts[0]) + (dy << shifts[1]) + (dz << shifts[2])
        pos = torch.searchsorted(skeys, target).clamp(max=n - 1)
        found = skeys[pos] == target
        rows.append(arange[found])
        nbrs.append(order[pos[found]])
        offs.append(torch.full_like(rows[-1], o))
    row, nbr, off = torch.cat(rows), torch.cat(nbrs), torch.cat(offs)
    _refuse(0, row.numel())
    by = torch.sort(row * (k ** 3) + off).indices
    row, nbr, off = row[by], nbr[by], off[by]
    counts = torch.bincount(row, minlength=n)
    rowptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    return KernelMap(n, k, d, rowptr.int(), nbr.int(), off.int(), row.int())


def build_kernel_map(coords, batch=None, kernel_size=3, dilation=1, stride=1, transposed=False):
    """The kernel map of a stride-1 sparse convolution over ``coords`` [N, 3] (x, y, z; integers,
    or floats holding integers) of the batch items ``batch`` [N] (optional).  Refused, each with
    a message: even kernel sizes, stride != 1, transposed, duplicate (batch, coords) rows,
    non-integer coords, a padded key beyond 63 bits, 2^31 voxels or pairs or more."""
    check_stride(stride, transposed)
    k, d = _kernel_size(kernel_size), _dilation(dilation)
    n, coords, batch = _check_coords(coords, batch)
    if not coords.is_cuda:
        return _map_torch(coords, batch, n, k, d)
    from .ops import _workspace
    dev = coords.device
    L = _lib.lib
    stream = _lib.stream_ptr(dev)
    if coords.is_floating_point():
        if bool((coords.abs() > 2147483520.0).any()):
            raise ValueError("a coordinate does not fit 32 bits")
    elif coords.dtype == torch.int64:
        if bool((coords.abs() > _INT32_MAX - 1).any()):
            raise ValueError("a coordinate does not fit 32 bits")
    c32 = _lib.dense(coords, torch.int32)
    if batch is not None:
        _lib.require_cuda(batch)
        batch = _lib.dense(batch, torch.int64, 8)
    record = torch.empty(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = L.spt_sparse_bounds_i32(_lib.ptr(c32), _lib.ptr(batch), n, _lib.ptr(record), stream)
    _lib.check(st, "spt_sparse_bounds_i32")
    rec = record.tolist()                                           # host read 1: the bounds
    mins, maxs = rec[0:8:2], rec[1:8:2]
    if batch is None:
        mins[3] = maxs[3] = 0
    origin, bits, total = _key_layout(mins, maxs, (k // 2) * d)
    if total == 0:
        bits[0], total = 1, 1                                        # one voxel: a 1-bit key
    c_origin = (_lib._c.c_int64 * 4)(*origin)
    c_bits = (_lib._c.c_int * 4)(*bits)
    skeys = torch.empty(n, dtype=torch.int64, device=dev)
    sorder = torch.empty(n, dtype=torch.int32, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    record2 = torch.empty(2, dtype=torch.int64, device=dev)
    nbytes = L.spt_sparse_map_count_workspace_bytes(n, total)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_sparse_map_count(_lib.ptr(c32), _lib.ptr(batch), n, c_origin, c_bits, k, d,
                                    _lib.ptr(skeys), _lib.ptr(sorder), _lib.ptr(rowptr),
                                    _lib.ptr(record2), _lib.ptr(ws), nbytes, stream)
    _lib.check(st, "spt_sparse_map_count")
    pairs, dups = record2.tolist()                                  # host read 2: pairs, duplicates
    _refuse(dups, pairs)
    nbr = torch.empty(pairs, dtype=torch.int32, device=dev)
    off = torch.empty(pairs, dtype=torch.int32, device=dev)
    row = torch.empty(pairs, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = L.spt_sparse_map_fill(_lib.ptr(c32), _lib.ptr(batch), n, c_origin, c_bits, k, d,
                                   _lib.ptr(skeys), _lib.ptr(sorder), _lib.ptr(rowptr), pairs,
                                   _lib.ptr(nbr), _lib.ptr(off), _lib.ptr(row), stream)
    _lib.check(st, "spt_sparse_map_fill")
    return KernelMap(n, k, d, rowptr, nbr, off, row)


def kernel_supported(c_in, c_out):
    """Whether the HIP forward takes (C_in, C_out): C_in 1 .. 64, C_out a multiple of 16 up to 64."""
    return bool(_lib.lib.spt_sparse_conv_supported(int(c_in), int(c_out)))


def _fwd_device(x, w, bias, kmap, flip):
    """out [n, w.shape[2]] f32 of the forward kernel on dense f32 operands."""
    n, ci = x.shape
    k3, _, co = w.shape
    dev = x.device
    out = torch.empty((n, co), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_sparse_conv_fwd_f32(_lib.ptr(x), n, ci, _lib.ptr(w), k3, co, _lib.ptr(bias),
                                              _lib.ptr(kmap.rowptr), _lib.ptr(kmap.nbr),
                                              _lib.ptr(kmap.off), int(flip), _lib.ptr(out),
                                              _lib.stream_ptr(dev))
    _lib.check(st, "spt_sparse_conv_fwd_f32")
    return out


class _SparseConv3d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, kmap):
        x2 = _lib.dense(x.detach(), torch.float32)
        w = _lib.dense(weight.detach(), torch.float32).view(kmap.k3, x2.shape[1], -1)
        b = None if bias is None else _lib.dense(bias.detach(), torch.float32)
        out = _fwd_device(x2, w, b, kmap, 0)
        ctx.save_for_backward(x2, w)
        ctx.kmap, ctx.wshape = kmap, tuple(weight.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        from .ops import _workspace
        x, w = ctx.saved_tensors
        kmap = ctx.kmap
        n, ci = x.shape
        k3, _, co = w.shape
        dev = x.device
        g = _lib.dense(gout, torch.float32)
        L = _lib.lib
        stream = _lib.stream_ptr(dev)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # pair (i, o, j) implies (j, K^3 - 1 - o, i): the same map, mirrored weight index
            dx = _fwd_device(g, w.transpose(1, 2).contiguous(), None, kmap, 1)
        if ctx.needs_input_grad[1]:
            perm, optr = kmap.by_offset()
            dw = torch.empty((k3, ci, co), dtype=torch.float32, device=dev)
            nbytes = L.spt_sparse_conv_dw_workspace_bytes(k3, ci, co)
            ws = _workspace(nbytes, dev)
            with torch.cuda.device(dev):
                st = L.spt_sparse_conv_dw_f32(_lib.ptr(x), _lib.ptr(g), n, ci, co, k3,
                                              _lib.ptr(kmap.nbr), _lib.ptr(kmap.row), _lib.ptr(perm),
                                              _lib.ptr(optr), kmap.num_pairs, _lib.ptr(dw),
                                              _lib.ptr(ws), nbytes, stream)
            _lib.check(st, "spt_sparse_conv_dw_f32")
            dw = dw.view(ctx.wshape)
        if ctx.needs_input_grad[2]:
            db = torch.empty(co, dtype=torch.float32, device=dev)
            nbytes = L.spt_sparse_conv_dbias_workspace_bytes(co)
            ws = _workspace(nbytes, dev)
            with torch.cuda.device(dev):
                st = L.spt_sparse_conv_dbias_f32(_lib.ptr(g), n, co, _lib.ptr(db), _lib.ptr(ws),
                                                 nbytes, stream)
            _lib.check(st, "spt_sparse_conv_dbias_f32")
        return dx, dw, db, None


def _conv_torch(x, weight, kmap, bias):
    """Per offset, ascending: gather -> matmul -> index_add_ (autograd differentiates it)."""
    n, ci = x.shape
    w = weight.reshape(kmap.k3, ci, -1)
    co = w.shape[2]
    perm, optr = kmap.by_offset_torch()
    nbr, row = kmap.nbr.long(), kmap.row.long()
    out = x.new_zeros((n, co))
    if bias is not None:
        out = out + bias
    bounds = optr.tolist()                                          # host read on device tensors
    for o in range(kmap.k3):
        b, e = bounds[o], bounds[o + 1]
        if e > b:
            sel = perm[b:e]
            out = out.index_add(0, row[sel], x[nbr[sel]] @ w[o])
    return out


def sparse_conv3d(x, weight, kmap, bias=None):
    """``x`` [N, C_in], ``weight`` [K^3, C_in, C_out] (K = 1: [C_in, C_out]), ``kmap`` of
    ``build_kernel_map`` over the same N voxels, ``bias`` [C_out] optional -> [N, C_out], with
    gradients for x, weight and bias."""
    if x.dim() != 2 or x.shape[0] != kmap.n:
        raise ValueError(f"x must be [{kmap.n}, C_in], got {tuple(x.shape)}")
    ci = x.shape[1]
    want = (ci,) if kmap.k3 == 1 and weight.dim() == 2 else (kmap.k3, ci)
    if tuple(weight.shape[:-1]) != want or weight.dim() not in (2, 3):
        raise ValueError(f"weight must be [{kmap.k3}, {ci}, C_out] ([{ci}, C_out] for K = 1), got "
                         f"{tuple(weight.shape)}")
    co = weight.shape[-1]
    if bias is not None and tuple(bias.shape) != (co,):
        raise ValueError(f"bias must be [{co}], got {tuple(bias.shape)}")
    if x.device != kmap.device:
        raise ValueError(f"x is on {x.device}, the kernel map on {kmap.device}")
    if (x.is_cuda and not _FORCE_COMPOSITION and x.dtype == torch.float32
            and weight.dtype == torch.float32 and kernel_supported(ci, co)):
        return _SparseConv3d.apply(x, weight, bias, kmap)
    return _conv_torch(x, weight, kmap, bias)
