"""Plain torch CPU restatement of ``GridSampling3D`` (src/transforms/sampling.py:86-468), shared
by tests/golden/make_golden_grid_sampling.py, tests/test_grid_sampling_reference_cpu.py and
tests/test_grid_sampling_gpu.py.  It imports nothing of the package under test.

Rules restated (see the transform's docstring in the package for the list): voxel coordinates
``torch.round(pos / size)``; voxel ids from ``grid_cluster`` / ``voxel_grid`` relabelled by
``consecutive_cluster``; the representative of a voxel is its HIGHEST point index (PyG's
``scatter_`` of an arange on the CPU); means are ``index_add_`` sums in point order divided by the
float count (``dtype=torch.float64`` computes them in f64 from the same f32 inputs); histograms,
votes (ties to the lowest label), ``sub`` and ``obj`` as ``_group_data`` builds them.

``grid_cluster`` and ``voxel_grid`` below are restatements of the PUBLISHED rule of torch_cluster
/ torch_geometric ("[third-party restated]", like the oracle's): neither library is installed
where this suite is developed, so the restatement cannot be pinned on them.  Only the ORDER of
their ids survives ``consecutive_cluster``, and that order is the lexicographic order of
``(batch, z, y, x)``.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_sampling.npz")

SIZE = 0.25
FINE_SIZE = 0.03
NUM_BINS = 14
VOTING_KEYS = ("y", "super_index", "is_val")
INSTANCE_KEYS = ("obj", "obj_pred")
CLUSTER_KEYS = ("sub",)
LAST_KEYS = ("batch", "node_id")
NORMAL_KEYS = ("normal",)

# the keys of the fixture's cloud, in stored order (obj in front of y: _group_data reads data.y
# while it builds obj)
INPUT_KEYS = ("pos", "rgb", "intensity", "normal", "obj", "y", "is_val", "sub", "other")
MEAN_KEYS = ("pos", "rgb", "intensity", "normal")

# case -> (constructor arguments, with_batch)
CASES = {
    "default": (dict(size=SIZE, hist_key="y", hist_size=NUM_BINS), False),
    "batch": (dict(size=SIZE, hist_key="y", hist_size=NUM_BINS), True),
    "vote": (dict(size=SIZE), False),
    "quant": (dict(size=SIZE, quantize_coords=True, hist_key="y", hist_size=NUM_BINS), False),
    "quant_neg": (dict(size=SIZE, quantize_coords=True, allow_negative_coords=True,
                       hist_key="y", hist_size=NUM_BINS), False),
    "last": (dict(size=SIZE, mode="last"), False),
    "fine": (dict(size=FINE_SIZE, hist_key="y", hist_size=NUM_BINS), False),
}


def grid_cluster(pos, size):
    """torch_cluster.grid_cluster(pos, size) with start / end = None  [third-party restated]:
    sum_d long((pos_d - min_d) / size_d) * prod_{j<d} (long((max_j - min_j) / size_j) + 1)."""
    start, end = pos.min(dim=0).values, pos.max(dim=0).values
    c = ((pos - start) / size).long()
    num = ((end - start) / size).long() + 1
    stride = torch.cat([num.new_ones(1), num.cumprod(0)[:-1]])
    return (c * stride).sum(dim=1)


def voxel_grid(pos, size, batch):
    """torch_geometric.nn.pool.voxel_grid(pos, size, batch)  [third-party restated]: the batch
    index becomes a last coordinate of voxel size 1."""
    pos = torch.cat([pos, batch.view(-1, 1).to(pos.dtype)], dim=1)
    size = torch.tensor([float(size)] * 3 + [1.0], dtype=pos.dtype)
    return grid_cluster(pos, size)


def consecutive_cluster(src):
    """torch_geometric's consecutive_cluster  [third-party restated]: dense relabelling in sorted
    order; perm = the LAST position of each label (CPU scatter_ of an arange)."""
    unique, inv = torch.unique(src, sorted=True, return_inverse=True)
    # `perm[inv] = arange` keeps the last writer only when torch runs it on ONE thread (with
    # several the winner changes from run to run: seen while building the fixture, which is
    # therefore generated single-threaded); the rule itself, thread-proof:
    perm = torch.zeros(unique.numel(), dtype=torch.long)
    perm.scatter_reduce_(0, inv, torch.arange(inv.numel()), "amax", include_self=True)
    return inv, perm


def voxelize(pos, size, batch=None):
    """(coords [N, 3] f32 whole numbers, cluster [N], unique_pos_indices [V])."""
    coords = torch.round(pos / size)
    if batch is None:
        cluster = grid_cluster(coords, torch.ones(3))
    else:
        cluster = voxel_grid(coords, 1, batch)
    cluster, perm = consecutive_cluster(cluster)
    return coords, cluster, perm


def lexicographic_cluster(coords, batch=None):
    """The same relabelling from the stated order alone: rank of (batch, z, y, x)."""
    c = coords.long()
    cols = [c[:, 0], c[:, 1], c[:, 2]] + ([batch.long()] if batch is not None else [])
    key = torch.zeros(c.shape[0], dtype=torch.int64)
    mult = 1
    for v in cols:
        key += (v - v.min()) * mult
        mult *= int(v.max() - v.min()) + 1
    return torch.unique(key, sorted=True, return_inverse=True)[1]


def scatter_mean(x, cluster, num, dtype=None):
    x = x if dtype is None else x.to(dtype)
    out = torch.zeros((num,) + tuple(x.shape[1:]), dtype=x.dtype)
    out.index_add_(0, cluster, x)
    cnt = torch.bincount(cluster, minlength=num).clamp(min=1).view((-1,) + (1,) * (x.dim() - 1))
    if x.is_floating_point():
        return out / cnt.to(x.dtype)
    return torch.div(out, cnt, rounding_mode="floor")


def histogram(labels, cluster, num, n_bins):
    assert bool(((labels >= 0) & (labels < n_bins)).all())
    return torch.bincount(cluster * n_bins + labels.long(), minlength=num * n_bins).view(num, n_bins)


def group_sub(cluster, item):
    """Cluster(cluster, item, dense=True): (pointers, points); points of a voxel in the order
    of a stable sort, i.e. ascending point index."""
    order = torch.sort(cluster, stable=True).indices
    counts = torch.bincount(cluster)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]), item[order]


def group_obj(cluster, obj, count, y):
    """InstanceData(cluster, obj, count, y, dense=True): (pointers, obj, count, y)."""
    key = cluster * (obj.max() + 1) + obj
    inv, perm = consecutive_cluster(key)
    merged = torch.zeros(perm.numel(), dtype=torch.long).index_add_(0, inv, count)
    sizes = torch.bincount(cluster[perm])
    return torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]), obj[perm], merged, y[perm]


def grid_sampling(fields, size, mode="mean", hist_key=None, hist_size=None, quantize_coords=False,
                  allow_negative_coords=False, dtype=None):
    """``fields``: dict of the cloud's keys in stored order.  Returns a dict: tensors, ``sub`` as
    ``(pointers, points)``, ``obj`` as ``(pointers, obj, count, y)``.  ``mode='last'`` takes the
    identity for the reference's shuffle.  ``dtype``: compute the means in that type."""
    bins = {} if hist_key is None else {hist_key: hist_size}
    pos = fields["pos"]
    n = pos.shape[0]
    coords, cluster, perm = voxelize(pos, size, fields.get("batch"))
    num = perm.numel()
    out = dict(fields)
    for key, item in fields.items():
        if key in INSTANCE_KEYS:
            y = out["y"] if out.get("y") is not None else torch.zeros_like(item)
            out[key] = group_obj(cluster, item, torch.ones_like(item), y)
            continue
        if key in CLUSTER_KEYS:
            out[key] = group_sub(cluster, item)
            continue
        if not torch.is_tensor(item) or item.size(0) != n:
            continue
        if mode == "last" or key in LAST_KEYS:
            out[key] = item[perm]
            continue
        is_bool = item.dtype == torch.bool
        if is_bool:
            item = item.int()
        if key in VOTING_KEYS or key in bins:
            voting = key not in bins
            n_bins = int(item.max()) + 1 if voting else bins[key]
            h = histogram(item, cluster, num, n_bins)
            out[key] = h.argmax(dim=-1) if voting else h
        else:
            out[key] = scatter_mean(item, cluster, num, dtype if item.is_floating_point() else None)
        if key in NORMAL_KEYS:
            out[key] = out[key] / out[key].norm(dim=1).view(-1, 1)
        if is_bool:
            out[key] = out[key].bool()
    if quantize_coords:
        c = coords[perm].int()
        if not allow_negative_coords:
            c = c - torch.min(c, dim=0, keepdim=True).values
        out["coords"] = c
    out["grid_size"] = torch.tensor([size])
    out["_cluster"], out["_perm"] = cluster, perm
    return out


# ---- the fixture -------------------------------------------------------------------------------
def load_golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def golden_fields(g, with_batch=False):
    """The fixture's cloud as a dict of tensors in stored order."""
    f = {k: torch.from_numpy(g[f"in__{k}"]) for k in INPUT_KEYS}
    if with_batch:
        f["batch"] = torch.from_numpy(g["in__batch"])
    return f


def flatten(out, case, keys=None):
    """Result dict -> {"case__key": array} with CSR objects spread over their parts."""
    flat = {}
    for k, v in out.items():
        if k.startswith("_") or (keys is not None and k not in keys):
            continue
        if isinstance(v, tuple) and len(v) == 2:
            flat[f"{case}__{k}__pointers"], flat[f"{case}__{k}__points"] = v
        elif isinstance(v, tuple):
            for name, t in zip(("pointers", "obj", "count", "y"), v):
                flat[f"{case}__{k}__{name}"] = t
        else:
            flat[f"{case}__{k}"] = v
    return {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in flat.items()}


# what each case keeps in the fixture (None: every key)
CASE_KEYS = {
    "default": None, "batch": None,
    "vote": ("y", "is_val"),
    "quant": ("coords",), "quant_neg": ("coords",),
    "last": ("pos", "rgb", "y", "is_val", "normal", "sub", "grid_size"),
    "fine": ("pos", "sub", "y"),
}


def canonical_sub(pointers, points):
    """The points of every voxel in ascending order.  The reference builds ``sub`` with an
    UNSTABLE ``indices.sort()`` (src/utils/sparse.py indices_to_pointers), so the order inside a
    voxel is whatever that sort left (and follows the shuffle in ``mode='last'``); nothing reads
    it.  The package and the restatement keep it ascending; comparisons go through this."""
    pointers, points = torch.as_tensor(pointers), torch.as_tensor(points)
    vox = torch.repeat_interleave(torch.arange(pointers.numel() - 1), pointers[1:] - pointers[:-1])
    assert bool((vox[1:] >= vox[:-1]).all())
    order = torch.sort(vox * (int(points.max()) + 1) + points).indices
    return points[order]


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def relative_deviation(x, ref64):
    """max |x - ref| / max |ref|, the suite's error figure."""
    x, ref64 = np.asarray(x, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    return float(np.abs(x - ref64).max() / np.abs(ref64).max())
