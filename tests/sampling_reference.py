"""numpy restatement of the per-segment sampler ``spt_sparse_sample`` (include/spt_hip.h), the
host twin the device draw is pinned to bit for bit.  Written from the specification of the
draw, not from the kernels; nothing is imported from the package.  Integers only, apart from the
count heuristic, which is evaluated as the reference does (src/utils/sparse.py:168-205): torch
f32 on the host.  The generator is ``rand32`` of tests/augment_reference.py.

    key[i]    = rand32(seed, i)                                    i in [0, n)
    order1    = stable argsort of key, ascending, unsigned         (the shuffle)
    bucket[p] = idx[order1[p]]  if 0 <= idx < num_seg and (mask is None or mask[order1[p]])
                else num_seg                                       (tail bucket, never drawn)
    order2    = order1[stable argsort of bucket]
    kept[s]   = population of bucket s
    size[s]   = number of i with idx[i] == s (mask ignored) when a mask is given, else kept[s]
    cnt[s]    = min(max(heuristic(size[s]), n_min), size[s], kept[s])
    heuristic = floor(f32(n_max) * tanh_f32(f32(size) / f32(n_max)))          n_max > 0
              = round_half_even(sqrt_f32(f32(size)))                          n_max <= 0
    ptr       = exclusive cumsum of cnt, length num_seg + 1
    out[ptr[s] + j] = order2[first position of bucket s + j]       j < cnt[s]
"""
import numpy as np
import torch

from augment_reference import rand32

SORT_TILE = 4096      # keys per workgroup of the device sorter
WAVE_CHUNK = 1024     # consecutive keys ranked by one wave

# the whole-permutation case of tests/test_sampling_gpu.py: one segment drawn entirely, so the
# output is the stable key-sorted order itself; about n^2 / 2^33 = 128 tied keys are expected
PERMUTATION_N = 1 << 20
PERMUTATION_SEED = 20


def keys(seed, n):
    """uint32 shuffle keys of the n positions."""
    return rand32(seed, np.arange(n, dtype=np.uint64)).astype(np.uint32)


def tied_keys(seed, n):
    """Number of positions whose key equals that of an earlier position."""
    return int(n - np.unique(keys(seed, n)).size)


def heuristic(size, n_max):
    """int64 array: how many samples a segment of ``size`` elements asks for, before the clamps
    (sparse.py:168-178, the same torch expressions on the host)."""
    size = torch.from_numpy(np.ascontiguousarray(size, dtype=np.int64))
    if n_max > 0:
        ns = (n_max * torch.tanh(size / n_max)).floor().long()
    else:
        ns = size.sqrt().round().long()
    return ns.numpy()


def correctly_rounded_heuristic(size, n_max):
    """The n_max > 0 heuristic with tanh evaluated in f64 and rounded once to f32."""
    x = np.asarray(size, dtype=np.float32) / np.float32(n_max)
    t = np.tanh(x.astype(np.float64)).astype(np.float32)
    return np.floor(np.float32(n_max) * t).astype(np.int64)


def as_bool_mask(mask, n):
    """None, a boolean [n] array or an array of positions -> None or boolean [n]."""
    if mask is None:
        return None
    mask = np.asarray(mask)
    if mask.dtype == np.bool_:
        assert mask.shape == (n,)
        return mask
    out = np.zeros(n, dtype=np.bool_)
    out[mask.astype(np.int64)] = True
    return out


def sample_counts(idx, n_max, n_min, mask=None, num_segments=None):
    """(cnt [S], kept [S]) int64."""
    idx = np.asarray(idx, dtype=np.int64)
    n = idx.size
    if num_segments is None:
        num_segments = int(idx.max()) + 1 if n else 1
    mask = as_bool_mask(mask, n)
    inside = (idx >= 0) & (idx < num_segments)
    keep = inside if mask is None else inside & mask
    kept = np.bincount(idx[keep], minlength=num_segments).astype(np.int64)
    size = kept if mask is None else np.bincount(idx[inside], minlength=num_segments).astype(np.int64)
    cnt = np.minimum(np.minimum(np.maximum(heuristic(size, n_max), n_min), size), kept)
    return cnt, kept


def sparse_sample(idx, n_max=32, n_min=1, seed=0, mask=None, num_segments=None):
    """(samples [ptr[-1]] int64, ptr [S + 1] int64) as torch tensors."""
    idx = np.asarray(idx, dtype=np.int64)
    n = idx.size
    if num_segments is None:
        num_segments = int(idx.max()) + 1 if n else 1
    mask = as_bool_mask(mask, n)
    cnt, kept = sample_counts(idx, n_max, n_min, mask, num_segments)
    ptr = np.zeros(num_segments + 1, dtype=np.int64)
    np.cumsum(cnt, out=ptr[1:])

    order1 = np.argsort(keys(seed, n), kind="stable")
    shuffled = idx[order1]
    keep = (shuffled >= 0) & (shuffled < num_segments)
    if mask is not None:
        keep &= mask[order1]
    bucket = np.where(keep, shuffled, num_segments)
    order2 = order1[np.argsort(bucket, kind="stable")]
    first = np.zeros(num_segments + 1, dtype=np.int64)          # first position of bucket s
    np.cumsum(kept, out=first[1:])

    seg = np.repeat(np.arange(num_segments, dtype=np.int64), cnt)
    j = np.arange(int(ptr[-1]), dtype=np.int64) - ptr[seg]
    out = order2[first[seg] + j]
    return torch.from_numpy(out.astype(np.int64)), torch.from_numpy(ptr)
