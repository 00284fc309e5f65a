"""``PointFeatures`` (src/transforms/point.py:41-182) and the ``AddKeysTo`` that follows it in the
preprocessing chain (src/transforms/data.py:221-249), on the kernels of ``csrc/point_feat.hip``
(colour keys, density) and the existing ``neighbors.geometric_features`` (eigenfeatures).

``point_colors`` / ``point_density`` are the two kernels' wrappers; ``point_features`` is the body
of ``PointFeatures._process``; ``partition_input`` is ``PointFeatures`` + ``AddKeysTo(to='x',
delete_after=False)`` in one go, with the colour kernel writing its columns of ``x`` directly.

Device tensors only: a CPU tensor raises ``RuntimeError`` (there is no torch composition behind
these functions).  ``Data.add_keys_to`` / ``transforms.AddKeysTo`` are plain tensor bookkeeping
and work on any device.  No function here reads anything back to the host."""
import torch

from . import _lib

__all__ = ["RADIOMETRIC_FEATURES", "GEOMETRIC_FEATURES", "POINT_FEATURES", "GEOF_SLICES",
           "sanitize_keys", "point_colors", "point_density", "point_features",
           "partition_input"]

# src/utils/keys.py:17-37
RADIOMETRIC_FEATURES = ["rgb", "hsv", "lab", "intensity"]
GEOMETRIC_FEATURES = ["linearity", "planarity", "scattering", "verticality", "curvature",
                      "length", "surface", "volume", "normal"]
POINT_FEATURES = ["density", "elevation", "pos_room"] + GEOMETRIC_FEATURES + RADIOMETRIC_FEATURES

# columns of the [N, 11] eigenfeature table per key (src/utils/geometry.py:165-174)
GEOF_SLICES = {"linearity": (0, 1), "planarity": (1, 2), "scattering": (2, 3),
               "verticality": (3, 4), "normal": (4, 7), "length": (7, 8), "surface": (8, 9),
               "volume": (9, 10), "curvature": (10, 11)}

_COLOR_BITS = {"rgb": 1, "hsv": 2, "lab": 4}


def sanitize_keys(keys, default=()):
    """Sorted tuple of unique keys; a string is one key, anything that is not iterable
    (``None``) gives ``default`` (src/utils/keys.py:66-86)."""
    if isinstance(keys, str):
        out = [keys]
    else:
        try:
            out = list(keys)
        except TypeError:
            out = list(default)
    if not all(isinstance(k, str) for k in out):
        raise ValueError(f"keys must be a string or an iterable of strings, got {keys!r}")
    return tuple(sorted(set(out)))


def _rgb_input(rgb):
    _lib.require_cuda(rgb)
    if rgb.dim() != 2 or rgb.shape[1] != 3:
        raise ValueError(f"rgb must be [N, 3], got {tuple(rgb.shape)}")
    rgb = rgb.detach()
    if rgb.dtype not in (torch.uint8, torch.float32):
        rgb = rgb.float()                                   # what to_float_rgb starts with
    return rgb.contiguous()


def _color_block(out, n, key):
    """(pointer, row stride in floats) of an [n, 3] f32 destination whose rows are contiguous."""
    if out.dtype != torch.float32 or tuple(out.shape) != (n, 3) or not out.is_cuda:
        raise ValueError(f"out[{key!r}] must be a [{n}, 3] float32 device tensor")
    if n > 0 and out.stride(1) != 1:
        raise ValueError(f"out[{key!r}]: the three columns must be adjacent in memory")
    ld = out.stride(0) if n > 1 else 3
    if ld < 3:
        raise ValueError(f"out[{key!r}]: rows overlap")
    return out.data_ptr(), int(ld)


def point_colors(rgb, keys=("rgb", "hsv", "lab"), out=None):
    """``{key: [N, 3] f32}`` for the requested keys among ``rgb`` (``to_float_rgb``: [0, 1]
    floats), ``hsv`` (``rgb2hsv`` with the hue / 360) and ``lab`` (``rgb2lab`` / 100), as
    ``PointFeatures`` stores them, in one pass over ``rgb`` [N, 3] uint8 or float (other dtypes
    are cast to float first, like the reference's ``rgb.float()``).

    ``out``: ``{key: tensor}`` destinations, each [N, 3] f32 with adjacent columns and any row
    stride - e.g. ``x[:, 2:5]`` of a wider table; missing ones are allocated.  A destination must
    not share memory with ``rgb``.  The values do not depend on where they are written."""
    from .ops import _workspace
    if isinstance(keys, str):
        keys = (keys,)
    keys = tuple(dict.fromkeys(keys))
    bad = [k for k in keys if k not in _COLOR_BITS]
    if bad:
        raise ValueError(f"unknown colour keys {bad}: expected some of {list(_COLOR_BITS)}")
    src = _rgb_input(rgb)
    n = src.shape[0]
    dev = src.device
    res = {}
    for k in keys:
        t = out.get(k) if out else None
        res[k] = t if t is not None else torch.empty((n, 3), dtype=torch.float32, device=dev)
    if not keys or n == 0:
        return res
    mask = 0
    blocks = {}
    for k in keys:
        mask |= _COLOR_BITS[k]
        blocks[k] = _color_block(res[k], n, k)
    L = _lib.lib
    ws = _workspace(L.spt_point_color_workspace_bytes(n), dev)
    args = []
    for k in ("rgb", "hsv", "lab"):
        args += list(blocks.get(k, (None, 3)))
    with torch.cuda.device(dev):
        st = L.spt_point_color_f32(_lib.ptr(src), int(src.dtype == torch.uint8), n, mask, *args,
                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(st, "spt_point_color_f32")
    return res


def _knn_table(t, dtype, name):
    """A [N, k] table readable in place: unit column stride, rows ``ld`` elements apart."""
    _lib.require_cuda(t)
    if t.dim() != 2:
        raise ValueError(f"{name} must be [N, k], got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype != dtype:
        t = t.to(dtype)
    n, k = t.shape
    if n > 1 and k > 0 and (t.stride(1) != 1 or t.stride(0) < k):
        t = t.contiguous()
    elif n <= 1:
        t = t.contiguous()
    return t, (int(t.stride(0)) if n > 1 else k)


def point_density(neighbor_index, neighbor_distance):
    """``density`` [N, 1] f32 = (number of ``neighbor_index[n] >= 0``) / (max of
    ``neighbor_distance[n]``)^2 (point.py:158-161), IEEE f32: a row of -1 gives 0, a row whose
    largest distance is 0 gives inf.  Both [N, k] tables are read in place, also as column
    slices of wider tables (``knn_1``'s results).  1 <= k <= 255."""
    nn, ld_nn = _knn_table(neighbor_index, torch.int64, "neighbor_index")
    dist, ld_d = _knn_table(neighbor_distance, torch.float32, "neighbor_distance")
    if nn.shape != dist.shape:
        raise ValueError(f"neighbor_index {tuple(nn.shape)} and neighbor_distance "
                         f"{tuple(dist.shape)} differ in shape")
    n, k = nn.shape
    if not 1 <= k <= 255:
        raise ValueError(f"k must be in 1..255, got {k}")
    dev = nn.device
    out = torch.empty((n, 1), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        st = _lib.lib.spt_point_density_f32(_lib.ptr(nn), ld_nn, _lib.ptr(dist), ld_d, n, k,
                                            _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(st, "spt_point_density_f32")
    return out


def _keys_to_compute(data, keys, overwrite):
    keys = sanitize_keys(keys, default=POINT_FEATURES)
    todo = set(keys) if overwrite else set(keys) - set(data.keys)
    return keys, todo


def _geof_table(data, todo, k_min, k_step, k_min_search, add_self_as_neighbor):
    """The [N, 11] eigenfeature table when a geometric key is asked for (point.py:164-180)."""
    from .neighbors import geometric_features
    if not (todo & set(GEOMETRIC_FEATURES)) or data.pos is None:
        return None
    if data.neighbor_index is None:
        raise ValueError("Data is expected to have a 'neighbor_index' attribute")
    return geometric_features(data.pos, data.neighbor_index, k_min=k_min,
                              add_self_as_neighbor=add_self_as_neighbor, k_step=k_step,
                              k_min_search=k_min_search)


def _density_of(data):
    if data.neighbor_index is None or data.get("neighbor_distance") is None:
        raise ValueError("'density' needs data.neighbor_index and data.neighbor_distance")
    return point_density(data.neighbor_index, data.neighbor_distance)


def point_features(data, keys=None, k_min=5, k_step=-1, k_min_search=25,
                   add_self_as_neighbor=True, overwrite=True):
    """``PointFeatures._process`` on ``data`` (a ``Data`` on the device), in place.

    ``keys``: ``None`` = the reference's ``POINT_FEATURES``.  ``overwrite=False`` leaves the
    keys ``data`` already holds alone, except ``rgb``, which is always brought to [0, 1] floats.
    The colour keys need ``data.rgb`` and are skipped without it; ``density`` needs
    ``neighbor_index`` / ``neighbor_distance``; the geometric keys come from
    ``neighbors.geometric_features`` on ``pos`` / ``neighbor_index`` (the spatial order a
    preceding ``knn_1`` left on ``pos`` is used as there) and are stored per key: [N, 1], and
    ``normal`` [N, 3], as views of one [N, 11] table.  Keys nothing here computes
    (``elevation``, ``pos_room``, ``intensity``) are ignored like in the reference."""
    keys, todo = _keys_to_compute(data, keys, overwrite)
    if data.rgb is not None:
        want = [k for k in ("rgb", "hsv", "lab") if (k in keys if k == "rgb" else k in todo)]
        for k, v in point_colors(data.rgb, want).items():
            data[k] = v
    if "density" in todo:
        data.density = _density_of(data)
    feats = _geof_table(data, todo, k_min, k_step, k_min_search, add_self_as_neighbor)
    if feats is not None:
        for k in todo & set(GEOMETRIC_FEATURES):
            lo, hi = GEOF_SLICES[k]
            data[k] = feats[:, lo:hi]
    return data


def partition_input(data, point_keys=None, partition_keys=None, to="x", k_min=5, k_step=-1,
                    k_min_search=25, add_self_as_neighbor=True, overwrite=True, strict=True):
    """``PointFeatures(point_keys, ...)`` followed by ``AddKeysTo(partition_keys, to=to,
    strict=strict, delete_after=False)`` with the table allocated once: ``x`` [N, F] holds the
    columns of ``partition_keys`` in their order (after an existing ``to``), the colour kernel
    writes its keys straight into their columns, density / eigenfeatures / keys computed
    elsewhere (``elevation``, a kept ``hsv``) are copied into theirs, and no ``torch.cat`` runs.
    Every key ``PointFeatures`` computed that is part of ``x`` is then stored on ``data`` as a
    VIEW of its columns of ``x`` (same values, shared memory); computed keys outside
    ``partition_keys`` get tensors of their own.  Bit for bit the two-step result."""
    keys, todo = _keys_to_compute(data, point_keys, overwrite)
    if isinstance(partition_keys, str):
        partition_keys = [partition_keys]
    pkeys = list(partition_keys) if partition_keys is not None else []
    if len(pkeys) != len(set(pkeys)):
        raise ValueError("partition_keys holds a key twice")
    has_rgb = data.rgb is not None
    colors = [k for k in ("rgb", "hsv", "lab")
              if has_rgb and (k in keys if k == "rgb" else k in todo)]
    feats = _geof_table(data, todo, k_min, k_step, k_min_search, add_self_as_neighbor)
    geof = sorted(todo & set(GEOMETRIC_FEATURES)) if feats is not None else []
    computed = set(colors) | set(geof) | ({"density"} & todo)

    # widths of the columns: computed keys from their definition, the others from data
    previous = data.get(to)
    n = previous.shape[0] if previous is not None else data.num_nodes
    layout, col = [], (0 if previous is None else
                       (1 if previous.dim() == 1 else previous.shape[1]))
    for k in pkeys:
        if k in computed:
            w = 3 if k in _COLOR_BITS or k == "normal" else 1
            src = None
        else:
            src = data.get(k)
            if src is None:
                if strict:
                    raise Exception(f"Data should contain the attribute '{k}'")
                continue
            if src.shape[0] != n:
                if previous is None:
                    raise Exception(f"Data should contain the attribute '{to}'")
                raise Exception(f"The tensors '{to}' and '{k}' can't be concatenated, "
                                f"'{to}': {n}, '{k}': {src.shape[0]}")
            src = src.unsqueeze(-1) if src.dim() == 1 else src
            w = src.shape[1]
        layout.append((k, col, w, src))
        col += w
    dev = data.pos.device if data.pos is not None else data.device
    x = torch.empty((n, col), dtype=torch.float32, device=dev) if pkeys else None
    if x is not None and previous is not None:
        x[:, :layout[0][1] if layout else col] = previous.unsqueeze(-1) if previous.dim() == 1 \
            else previous
    where = {k: x[:, c:c + w] for k, c, w, _ in layout}

    if colors:
        res = point_colors(data.rgb, colors, out={k: where[k] for k in colors if k in where})
        for k in colors:
            data[k] = res[k]
    if "density" in computed:
        d = _density_of(data)
        if "density" in where:
            where["density"].copy_(d)
            d = where["density"]
        data.density = d
    for k in geof:
        lo, hi = GEOF_SLICES[k]
        if k in where:
            where[k].copy_(feats[:, lo:hi])
            data[k] = where[k]
        else:
            data[k] = feats[:, lo:hi]
    for k, c, w, src in layout:
        if src is not None:
            where[k].copy_(src)
    if x is not None:
        data[to] = x
    return data
