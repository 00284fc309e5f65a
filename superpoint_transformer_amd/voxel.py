"""Voxel groups of a raw cloud and the per-voxel reductions of ``GridSampling3D``
(src/transforms/sampling.py:86-468) on the kernels of ``csrc/voxel.hip``.

``voxel_groups`` -> ``VoxelGroups`` (pointers, cluster, order, last, coords); ``group_mean``,
``group_histogram``, ``group_vote`` and ``group_last`` reduce point tensors over it.
``transforms.GridSampling3D`` strings them together key by key.

Rules (the reference's, where they differ from its docstrings):
  * integer coordinate = ``torch.round(pos / size)``: IEEE f32 division, round half to even;
  * voxels are numbered in lexicographic order of ``(batch, z, y, x)`` - the order that
    ``consecutive_cluster`` leaves of ``grid_cluster`` / ``voxel_grid``;
  * inside a voxel the points of ``order`` are ascending; ``last`` is the highest point index
    (what PyG's ``scatter_`` leaves on the CPU; unspecified on CUDA, fixed here);
  * a mean is the f32 sum in ascending point order from 0 divided by the float count (torch's
    CPU ``index_add_``); voxels of more than 512 points are summed on the device by a fixed
    64-lane tree instead, so every result is bitwise reproducible from run to run.

Host reads of ``voxel_groups`` on the device, two per call: the ten-number bounds record (sizes
the key and raises ``ValueError`` for a non-finite position or a key wider than 63 bits) and the
number of voxels V (sizes the outputs).  ``group_histogram`` / ``group_vote`` read one status
word back to raise on a label outside its range; ``group_vote`` also reads the label range.  This
is once-per-cloud preprocessing, not a captured step.

CPU tensors take a torch composition of the same rules (what the CPU tests run); so do value
tensors that are neither f32 nor integer (f64, f16 means), on either device."""
import torch

from . import _lib

__all__ = ["VoxelGroups", "voxel_groups", "group_mean", "group_histogram", "group_vote",
           "group_last", "MAX_KEY_BITS", "MAX_BINS"]

MAX_KEY_BITS = 63
MAX_BINS = 256
_INT32_MAX = (1 << 31) - 1


class VoxelGroups:
    """``pointers`` [V + 1] int64, ``cluster`` [N] int64 (voxel of every point), ``order`` [N]
    int64 (points sorted by voxel, ascending inside a voxel), ``last`` [V] int64 (highest point
    index of each voxel), ``coords`` [V, 3] int32 (x, y, z integer coordinates), ``size``."""
    __slots__ = ("pointers", "cluster", "order", "last", "coords", "size")

    def __init__(self, pointers, cluster, order, last, coords, size):
        self.pointers, self.cluster, self.order = pointers, cluster, order
        self.last, self.coords, self.size = last, coords, float(size)

    @property
    def num_voxels(self):
        return self.pointers.numel() - 1

    @property
    def num_points(self):
        return self.cluster.numel()

    @property
    def counts(self):
        return self.pointers[1:] - self.pointers[:-1]

    @property
    def device(self):
        return self.pointers.device


def _field_bits(lo, hi):
    return (int(hi) - int(lo)).bit_length()


def _key_layout(mins, maxs):
    """Field widths (x, y, z, batch) of the key and their sum; raises beyond 63 bits."""
    bits = [_field_bits(lo, hi) for lo, hi in zip(mins, maxs)]
    total = sum(bits)
    if total > MAX_KEY_BITS:
        raise ValueError(
            f"the voxel key needs {total} bits (x {bits[0]}, y {bits[1]}, z {bits[2]}, batch "
            f"{bits[3]}) for coordinates {list(zip(mins, maxs))}: more than {MAX_KEY_BITS}; a far "
            "outlier or a voxel size too small for the extent is the likely cause")
    return bits, total


def _check_inputs(pos, size, batch):
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must be [N, 3], got {tuple(pos.shape)}")
    n = pos.shape[0]
    if n > _INT32_MAX:
        raise ValueError("more than 2^31 - 1 points")
    if n == 0:
        raise ValueError("the cloud is empty")
    if not (float(size) > 0 and float(size) < float("inf")):
        raise ValueError(f"the voxel size must be positive and finite, got {size}")
    if batch is not None and (batch.dim() != 1 or batch.numel() != n):
        raise ValueError("batch must hold one index per point")
    return n


def _voxel_groups_torch(pos, size, batch):
    coords = torch.round(pos.float() / size)
    if not bool(torch.isfinite(coords).all()):
        raise ValueError("pos holds non-finite coordinates")
    if bool((coords.abs() > 2147483520.0).any()):
        raise ValueError("a voxel coordinate does not fit 32 bits")
    c = coords.long()
    cols = [c[:, 0], c[:, 1], c[:, 2]]
    if batch is not None:
        cols.append(batch.long())
    mins = [int(v.min()) for v in cols] + ([0] if batch is None else [])
    maxs = [int(v.max()) for v in cols] + ([0] if batch is None else [])
    if batch is not None and (mins[3] < -_INT32_MAX or maxs[3] > _INT32_MAX):
        raise ValueError("a batch index does not fit 32 bits")
    bits, _ = _key_layout(mins, maxs)
    key = torch.zeros(pos.shape[0], dtype=torch.int64, device=pos.device)
    shift = 0
    for v, lo, b in zip(cols, mins, bits):
        key |= (v - lo) << shift
        shift += b
    uniq, cluster, counts = torch.unique(key, sorted=True, return_inverse=True, return_counts=True)
    order = torch.sort(cluster, stable=True).indices
    pointers = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    last = order[pointers[1:] - 1]
    return VoxelGroups(pointers, cluster, order, last, c[last].int(), size)


def voxel_groups(pos, size, batch=None):
    """Voxels of ``pos`` [N, 3] f32 (a column block of a wider table works: only the row stride
    must be uniform) at voxel size ``size``, per cloud of ``batch`` [N] int64 when given.
    Returns a ``VoxelGroups``.  Raises ``ValueError`` for an empty cloud, more than 2^31 - 1
    points, a non-finite position, a coordinate beyond 32 bits and a key beyond 63 bits.

    On the device: two host reads (module docstring)."""
    n = _check_inputs(pos, size, batch)
    if not pos.is_cuda or pos.dtype != torch.float32:
        return _voxel_groups_torch(pos, size, batch)
    from .ops import _workspace
    dev = pos.device
    pos = pos.detach()
    if pos.stride(1) != 1 or pos.stride(0) < 3:
        pos = pos.contiguous()
    ld = pos.stride(0)
    if batch is not None:
        _lib.require_cuda(batch)
        batch = batch.detach().long().contiguous()
    L = _lib.lib
    stream = _lib.stream_ptr(dev)
    record = torch.empty(10, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = L.spt_voxel_bounds_f32(_lib.ptr(pos), n, ld, float(size), _lib.ptr(batch),
                                    _lib.ptr(record), stream)
    _lib.check(st, "spt_voxel_bounds_f32")
    rec = record.tolist()                                           # host read 1: the bounds
    if rec[8]:
        raise ValueError(f"pos holds {rec[8]} point(s) with a non-finite coordinate")
    if rec[9]:
        raise ValueError(f"{rec[9]} point(s) have a voxel coordinate or a batch index beyond 32 "
                         f"bits at size {size:g}")
    mins, maxs = rec[0:8:2], rec[1:8:2]
    bits, total = _key_layout(mins, maxs)
    total = max(total, 1)
    if sum(bits) == 0:
        bits[0] = 1                                                  # one voxel: a 1-bit key
    origin = (_lib._c.c_int64 * 4)(*mins)
    cbits = (_lib._c.c_int * 4)(*bits)
    pointers = torch.empty(n + 1, dtype=torch.int64, device=dev)
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    last = torch.empty(n, dtype=torch.int64, device=dev)
    coords = torch.empty((n, 3), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    nbytes = L.spt_voxel_groups_workspace_bytes(n, total)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_voxel_groups_f32(_lib.ptr(pos), n, ld, float(size), _lib.ptr(batch), origin,
                                    cbits, _lib.ptr(pointers), _lib.ptr(cluster), _lib.ptr(order),
                                    _lib.ptr(last), _lib.ptr(coords), _lib.ptr(count),
                                    _lib.ptr(ws), nbytes, stream)
    _lib.check(st, "spt_voxel_groups_f32")
    v = int(count.item())                                           # host read 2: V
    return VoxelGroups(pointers[:v + 1], cluster, order, last[:v], coords[:v], size)


def _check_rows(x, groups):
    if x.shape[0] != groups.num_points:
        raise ValueError(f"expected {groups.num_points} rows, got {x.shape[0]}")


def _mean_torch(x, groups, normalize):
    v = groups.num_voxels
    out = torch.zeros((v,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    out.index_add_(0, groups.cluster, x)
    cnt = groups.counts.clamp(min=1).view((-1,) + (1,) * (x.dim() - 1))
    if x.is_floating_point():
        out = out / cnt.to(x.dtype)
    else:
        out = torch.div(out, cnt, rounding_mode="floor")
    if normalize:
        out = out / out.norm(dim=1).view(-1, 1)
    return out


def group_mean(x, groups, normalize=False):
    """``scatter_mean(x, cluster, dim=0)`` of a ``[N]`` or ``[N, ...]`` tensor: the sum in
    ascending point order divided by the float count; integer tensors use floor division.
    ``normalize`` divides each ``[V, 3]`` row by its norm afterwards (the ``normal`` key; a zero
    mean gives NaN, like the reference).  f32 tensors of at most two dimensions on the device
    run on ``spt_voxel_mean_f32`` (any row stride, unit column stride), integer tensors on the
    integer segment-sum kernels; everything else takes the torch composition."""
    _check_rows(x, groups)
    if normalize and (x.dim() != 2 or x.shape[1] != 3):
        raise ValueError("normalize needs a [N, 3] tensor")
    if x.is_cuda and not x.is_floating_point() and x.dtype != torch.bool and not normalize:
        from .shims.scatter_shim import scatter_mean       # the integer segment-sum kernels
        return scatter_mean(x, groups.cluster, 0, None, groups.num_voxels)
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() <= 2 and x.numel()):
        return _mean_torch(x, groups, normalize)
    dev = x.device
    x = x.detach()
    n = x.shape[0]
    cols = 1 if x.dim() == 1 else x.shape[1]
    if x.dim() == 1:
        if x.stride(0) < 1:
            x = x.contiguous()
        ld = x.stride(0)
    else:
        if x.stride(1) != 1 or x.stride(0) < cols:
            x = x.contiguous()
        ld = x.stride(0)
    v = groups.num_voxels
    out = torch.empty((v,) if x.dim() == 1 else (v, cols), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_voxel_mean_f32(_lib.ptr(x), n, cols, ld, _lib.ptr(groups.pointers),
                                         _lib.ptr(groups.order), v, int(bool(normalize)),
                                         _lib.ptr(out), cols, _lib.stream_ptr(dev))
    _lib.check(st, "spt_voxel_mean_f32")
    return out


def _labels(labels, groups):
    _check_rows(labels, groups)
    if labels.dim() != 1 or labels.is_floating_point() or labels.is_complex():
        raise ValueError("labels must be a 1-D integer or boolean tensor")
    return labels.detach().long().contiguous()


def _hist_torch(labels, groups, n_bins):
    if bool(((labels < 0) | (labels >= n_bins)).any()):
        raise ValueError(f"a label lies outside [0, {n_bins})")
    v = groups.num_voxels
    flat = torch.bincount(groups.cluster * n_bins + labels, minlength=v * n_bins)
    return flat.view(v, n_bins)


def _hist_device(labels, groups, n_bins, vote):
    dev = labels.device
    v, n = groups.num_voxels, groups.num_points
    out = torch.empty((v,) if vote else (v, n_bins), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_voxel_hist_i64(_lib.ptr(labels), n, _lib.ptr(groups.pointers),
                                         _lib.ptr(groups.order), v, n_bins,
                                         None if vote else _lib.ptr(out),
                                         _lib.ptr(out) if vote else None, _lib.ptr(status),
                                         _lib.stream_ptr(dev))
    _lib.check(st, "spt_voxel_hist_i64")
    if int(status.item()):                                          # host read: the status word
        raise ValueError(f"a label lies outside [0, {n_bins})")
    return out


def group_histogram(labels, groups, n_bins):
    """``[V, n_bins]`` int64 label counts per voxel (``atomic_to_histogram`` with ``n_bins``
    given).  A label outside ``[0, n_bins)`` raises ``ValueError`` (the reference lets it spill
    into the next voxel's row).  On the device for ``n_bins <= 256``, the torch composition
    otherwise."""
    labels = _labels(labels, groups)
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError("n_bins must be positive")
    if not labels.is_cuda or n_bins > MAX_BINS:
        return _hist_torch(labels, groups, n_bins)
    return _hist_device(labels, groups, n_bins, vote=False)


def group_vote(labels, groups):
    """Majority label per voxel: the argmax of the histogram with ``n_bins = max + 1``, ties to
    the lowest label, without building the histogram.  Label ranges up to 256 run on the vote
    kernel; wider ones (``super_index``) relabel ``n_bins * cluster + label`` with the package's
    ``consecutive_cluster`` and take the first largest count of each voxel's run.  Negative
    labels raise ``ValueError`` (the reference asserts)."""
    labels = _labels(labels, groups)
    lo, hi = int(labels.min()), int(labels.max())                   # host read: the label range
    if lo < 0:
        raise ValueError("voting only supports non-negative labels")
    n_bins = hi + 1
    if labels.is_cuda and n_bins <= MAX_BINS:
        return _hist_device(labels, groups, n_bins, vote=True)
    v = groups.num_voxels
    key = groups.cluster * n_bins + labels
    if labels.is_cuda:
        from .instance import _consecutive
        inv, perm = _consecutive(key)
        pairs = key[perm]
    else:
        pairs, inv = torch.unique(key, sorted=True, return_inverse=True)
    counts = torch.bincount(inv, minlength=pairs.numel())
    vox, lab = pairs // n_bins, pairs % n_bins
    # pairs are sorted by (voxel, label): the first pair holding the voxel's largest count is the
    # lowest label among the ties
    best = torch.zeros(v, dtype=counts.dtype, device=counts.device)
    best.scatter_reduce_(0, vox, counts, "amax", include_self=True)
    pos = torch.arange(pairs.numel(), device=pairs.device)
    cand = torch.where(counts == best[vox], pos, torch.full_like(pos, pairs.numel()))
    first = torch.full((v,), pairs.numel(), dtype=pos.dtype, device=pos.device)
    first.scatter_reduce_(0, vox, cand, "amin", include_self=True)
    return lab[first]


def group_last(groups, seed=None):
    """One representative point per voxel, ``[V]`` int64.  ``seed=None``: the highest point
    index (``groups.last``).  With a 64-bit ``seed`` the representative is the point with the
    greatest ``(rand32(seed, point), point)`` of ``csrc/rng.hpp``'s counter stream at the
    LOGICAL point index: uniform over the voxel's points, like the reference's shuffle, without
    an ``[N]`` permutation."""
    if seed is None:
        return groups.last
    seed = int(seed) & ((1 << 64) - 1)
    v, n = groups.num_voxels, groups.num_points
    if groups.pointers.is_cuda:
        dev = groups.device
        out = torch.empty(v, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_voxel_last(_lib.ptr(groups.pointers), _lib.ptr(groups.order), n, v,
                                         seed, 1, _lib.ptr(out), _lib.stream_ptr(dev))
        _lib.check(st, "spt_voxel_last")
        return out
    from .augment import rand32
    points = torch.arange(n)
    # (priority, point) as one signed word: the priority biased by 2^31 keeps the u32 order
    prio = ((rand32(seed, points) - (1 << 31)) << 32) | points
    best = torch.full((v,), torch.iinfo(torch.int64).min, dtype=torch.int64)
    best.scatter_reduce_(0, groups.cluster, prio, "amax", include_self=True)
    return best & 0xFFFFFFFF
