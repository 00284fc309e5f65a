"""Per-batch on-device graph transforms of the hot path's "next" rows
(SURVEY.md 8f): on-the-fly horizontal edge features fused with the edge
symmetrisation and the self loops."""
import ctypes

import torch

from . import _lib

__all__ = ["horizontal_edge_features", "EDGE_FEATURE_COLUMNS", "NodeSize", "SampleSubNodes",
           "SampleSegments", "SampleEdges", "OnTheFlyHorizontalEdgeFeatures",
           "SampleRadiusSubgraphs", "OnTheFlyInstanceGraph", "segment_sampling_weights",
           "NAGRestrictSize", "MortonOrder", "morton_code", "PartitionAdjacency", "GroundElevation",
           "PointFeatures", "AddKeysTo", "NAGJitterKey", "RandomTiltAndRotate",
           "RandomAnisotropicScale", "RandomAxisFlip", "NAGDropoutColumns", "NAGDropoutRows",
           "NAGColorAutoContrast", "NAGColorDrop", "GeometricAugmentation", "FeatureAugmentation",
           "ColorAugmentation", "GridSampling3D", "SaveNodeIndex", "NAGSaveNodeIndex", "DataTo",
           "NAGRemoveKeys", "SegmentFeatures", "RadiusHorizontalGraph",
           "GreedyContourPriorPartition", "QuantizePointCoordinates", "PretrainedCNN", "KNN",
           "AdjacencyGraph", "RemoveKeys"]

EDGE_FEATURE_COLUMNS = [
    "mean_off_x", "mean_off_y", "mean_off_z", "std_off_x", "std_off_y", "std_off_z",
    "mean_dist", "angle_source", "angle_target", "normal_angle", "log_length",
    "log_surface", "log_volume", "log_size", "centroid_dir_x", "centroid_dir_y",
    "centroid_dir_z", "centroid_dist"]


def horizontal_edge_features(edge_index, edge_attr, pos, normal, log_length, log_surface,
                             log_volume, log_size, add_self_loops=True):
    """``OnTheFlyHorizontalEdgeFeatures`` (all default keys) + ``NAGAddSelfLoops``
    of one level (src/transforms/graph.py:1135-1277, 1419-1452) in one kernel.

    ``edge_index`` [2,E] trimmed edges, ``edge_attr`` [E,7] (f16 on disk: cast
    here like the reference's ``.float()``), node attributes of the level.
    Returns (edge_index [2, 2E(+N)], edge_attr [2E(+N), 18])."""
    _lib.require_cuda(edge_index, edge_attr, pos)
    dev = pos.device
    se = edge_index.long().contiguous()
    e, n = se.shape[1], pos.shape[0]

    def f32(t, cols=None):
        t = t.detach().float().contiguous()
        return t.view(n, cols) if cols else t.view(-1)

    ea7 = edge_attr.detach().float().contiguous()
    if ea7.shape != (e, 7):
        raise ValueError(f"edge_attr must be [E,7], got {tuple(ea7.shape)}")
    etot = 2 * e + (n if add_self_loops else 0)
    ei_out = torch.empty((2, etot), dtype=torch.int64, device=dev)
    ea_out = torch.empty((etot, 18), dtype=torch.float32, device=dev)
    args = [f32(pos, 3), f32(normal, 3), f32(log_length), f32(log_surface), f32(log_volume),
            f32(log_size)]
    with torch.cuda.device(dev):
        st = _lib.lib.spt_horizontal_edge_features_f32(
            _lib.ptr(se), e, n, _lib.ptr(ea7), *[_lib.ptr(a) for a in args],
            int(add_self_loops), _lib.ptr(ei_out), _lib.ptr(ea_out), _lib.stream_ptr(dev))
    _lib.check(st, "spt_horizontal_edge_features_f32")
    # host knowledge of the layout just written: [i<j | j>i (| loops)] with edge i mirrored at
    # i + e - the attention backward takes its by-target stream from it instead of a second sort
    # (csr.EdgeCSR; checked on the device).  A later transform that thins the list
    # (SampleEdges with n >= 0, NAGRestrictSize) builds a new tensor without the attribute.
    ei_out._spt_mirror_pairs = e
    return ei_out, ea_out


def vertical_edge_features(child, parent):
    """``_on_the_fly_vertical_edge_features`` with all default keys
    (src/transforms/graph.py:1335-1416): ``child`` / ``parent`` are level objects (Data or
    dicts) holding pos, normal, log_length, log_surface, log_volume, log_size, and
    ``child.super_index``.  Returns ``v_edge_attr`` [num_child, 9] (one kernel)."""
    def get(d, k):
        v = d[k] if isinstance(d, dict) else getattr(d, k)
        return v
    sup = get(child, "super_index").long().contiguous()
    _lib.require_cuda(sup)
    n = sup.numel()
    dev = sup.device
    keys = ("pos", "normal", "log_length", "log_surface", "log_volume", "log_size")
    cargs = [get(child, k).detach().float().contiguous() for k in keys]
    pargs = [get(parent, k).detach().float().contiguous() for k in keys]
    out = torch.empty((n, 9), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_vertical_edge_features_f32(
            _lib.ptr(sup), n, *[_lib.ptr(a) for a in cargs], *[_lib.ptr(a) for a in pargs],
            _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(st, "spt_vertical_edge_features_f32")
    return out


class DataTo:
    """``DataTo(device)`` (src/transforms/device.py:9-20), the first ``pre_transform`` of
    configs/datamodule/semantic/default.yaml: the ``Data`` itself when it already lives on
    ``device``, else a new ``Data`` whose tensors, ``Cluster`` and ``InstanceData`` were moved."""

    def __init__(self, device):
        self.device = device if isinstance(device, torch.device) else torch.device(device)

    def __call__(self, data):
        from .data import Data
        if data.device == self.device:
            return data
        out = Data()
        for key, item in data:
            out[key] = item.to(self.device) if hasattr(item, "to") else item
        out.num_nodes = data._num_nodes
        return out


class SaveNodeIndex:
    """``SaveNodeIndex(key)`` (src/transforms/sampling.py:56-69): ``data[key] = arange(N)`` on
    the data's device, to track nodes from the output back to the input; the default chain
    stores it as ``'sub'``, which ``GridSampling3D`` turns into the raw-point ``Cluster``."""

    DEFAULT_KEY = "node_id"

    def __init__(self, key=None):
        self.key = key if key is not None else self.DEFAULT_KEY

    def __call__(self, data):
        data[self.key] = torch.arange(0, data.pos.shape[0], device=data.device)
        return data


class NAGSaveNodeIndex(SaveNodeIndex):
    """``NAGSaveNodeIndex(key)`` (src/transforms/sampling.py:72-83): ``SaveNodeIndex`` on every
    level of a NAG, in place.  The multi-run inference puts it in front of the augmentations, so
    that the logits of a sampled or shuffled NAG find their rows of the input NAG again."""

    def __call__(self, nag):
        transform = SaveNodeIndex(key=self.key)
        for i_level in range(nag.num_levels):
            nag._list[i_level] = transform(nag._list[i_level])
        return nag


def _instance_data_dense_torch(cluster, obj, count, y):
    """``InstanceData(cluster, obj, count, y, dense=True)`` (src/data/instance.py:70-98) as a
    torch composition, for CPU tensors: duplicate (cluster, obj) pairs merged, counts summed,
    ``y`` of the last holder of each pair."""
    from .instance import InstanceData
    cluster, obj, count, y = (t.long() for t in (cluster, obj, count, y))
    key = cluster * (obj.max() + 1) + obj
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    # the LAST holder (an index_put_ with duplicates keeps it only on one thread: amax says it)
    perm = torch.zeros(uniq.numel(), dtype=torch.int64, device=key.device)
    perm.scatter_reduce_(0, inv, torch.arange(inv.numel(), device=key.device), "amax")
    merged = torch.zeros(uniq.numel(), dtype=torch.int64, device=key.device).index_add_(0, inv, count)
    index = cluster[perm]
    sizes = torch.bincount(index, minlength=int(index.max()) + 1)
    if not bool((sizes > 0).all()):
        raise AssertionError("Indices must be dense")
    pointers = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
    return InstanceData(pointers, obj[perm], merged, y[perm])


class GridSampling3D:
    """``GridSampling3D`` (src/transforms/sampling.py:86-468), the voxelisation that opens the
    preprocessing chain, with the reference's signature: ``voxel.voxel_groups`` on
    ``data.pos`` (and ``data.batch`` when present), then every key of ``data`` in stored order
    exactly as ``_group_data`` walks them:

      * ``obj`` / ``obj_pred``: ``InstanceData(cluster, item, ones, y or zeros, dense=True)``, or
        ``item.merge(cluster)`` for an ``InstanceData`` (``y`` is read from the data AS STORED
        at that moment, like the reference: keep ``obj`` in front of ``y``);
      * ``sub``: the ``Cluster`` of the item's values per voxel, built from the groups'
        ``pointers`` and ``order`` without a second sort; it must be a 1-D integer tensor;
      * any other ``Cluster`` / ``InstanceData`` and any key whose name holds ``edge``:
        ``NotImplementedError``;
      * non-tensors and tensors with another first dimension than ``num_nodes``: untouched;
      * ``mode='last'``, and ``batch`` / ``node_id`` in any mode: ``item[representative]``;
      * a key of ``hist_key``: ``[V, n_bins]`` int64 histogram; ``y`` / ``super_index`` /
        ``is_val`` otherwise: the majority label, ties to the lowest (bool goes through int and
        comes back as bool);
      * everything else: the mean (``voxel.group_mean``; integer tensors floor); ``normal`` is
        divided by its norm afterwards.

    The representative of a voxel is its highest point index in ``mode='mean'``.  In
    ``mode='last'`` the reference shuffles the cloud first; here the representative is drawn
    per voxel by ``voxel.group_last`` under a seed taken from torch's CPU generator
    (``torch.manual_seed`` makes it reproducible), uniform over the voxel's points like the
    shuffle; ``shuffle = False`` on the instance keeps the highest index instead.  The points of
    ``sub`` inside a voxel stay in ascending order (the reference's follow its shuffle; nothing
    reads that order).  ``quantize_coords`` stores the integer voxel coordinates as ``coords``
    [V, 3] int32, minus their column minimum unless ``allow_negative_coords``;
    ``grid_size = tensor([size])``.  ``chunk_size`` is accepted and ignored: it only bounds the
    reference's temporaries.  ``groups_`` keeps the last call's ``VoxelGroups``."""

    _VOTING_KEYS = ("y", "super_index", "is_val")
    _INSTANCE_KEYS = ("obj", "obj_pred")
    _CLUSTER_KEYS = ("sub",)
    _LAST_KEYS = ("batch", SaveNodeIndex.DEFAULT_KEY)
    _NORMAL_KEYS = ("normal",)

    def __init__(self, size, quantize_coords=False, allow_negative_coords=False, mode="mean",
                 hist_key=None, hist_size=None, inplace=False, chunk_size=10_000_000,
                 verbose=False):
        hist_key = [] if hist_key is None else hist_key
        hist_size = [] if hist_size is None else hist_size
        hist_key = [hist_key] if isinstance(hist_key, str) else hist_key
        hist_size = [hist_size] if isinstance(hist_size, int) else hist_size
        assert isinstance(hist_key, list)
        assert isinstance(hist_size, list)
        assert len(hist_key) == len(hist_size)
        assert mode in ("mean", "last")
        self.grid_size = size
        self.quantize_coords = quantize_coords
        self.allow_negative_coords = allow_negative_coords
        self.mode = mode
        self.bins = {k: v for k, v in zip(hist_key, hist_size)}
        self.inplace = inplace
        self.chunk_size = chunk_size
        self.shuffle = True
        self.groups_ = None

    def _instance(self, data, item, cluster):
        from .instance import InstanceData
        if isinstance(item, InstanceData):
            if item.device.type == "cuda":
                return item.merge(cluster)
            return _instance_data_dense_torch(cluster[item.indices], item.obj, item.count, item.y)
        y = data.y if data.get("y") is not None else torch.zeros_like(item)
        if y.shape != item.shape:
            raise ValueError(
                f"instance labels need one semantic label per point, but data.y is "
                f"{tuple(y.shape)}: store the instance key in front of 'y'")
        count = torch.ones_like(item)
        if item.is_cuda:
            return InstanceData(cluster, item, count, y, dense=True)
        return _instance_data_dense_torch(cluster, item, count, y)

    def __call__(self, data_in):
        import re
        from . import voxel
        from .data import Cluster
        from .instance import InstanceData
        from .segment import _draw_seed
        data = data_in if self.inplace else data_in.clone()
        groups = voxel.voxel_groups(data.pos, self.grid_size, data.get("batch"))
        self.groups_ = groups
        pick = groups.last
        if self.mode == "last" and self.shuffle:
            pick = voxel.group_last(groups, _draw_seed())
        num_nodes = data.num_nodes
        for key, item in data:
            if re.search("edge", key):
                raise NotImplementedError("Edges not supported. Wrong data type.")
            if key in self._INSTANCE_KEYS:
                data[key] = self._instance(data, item, groups.cluster)
                continue
            if key in self._CLUSTER_KEYS:
                if not (torch.is_tensor(item) and item.dim() == 1 and not item.is_floating_point()):
                    raise NotImplementedError(
                        f"Cannot merge '{key}' with data type: {type(item)} into a Cluster object. "
                        "Only supports 1D Tensor of integers.")
                data[key] = Cluster(groups.pointers, item[groups.order])
                continue
            if isinstance(item, (Cluster, InstanceData)):
                raise NotImplementedError(f"Cannot merge '{key}' with data type: {type(item)}")
            if not torch.is_tensor(item) or item.dim() == 0 or item.size(0) != num_nodes:
                continue
            if self.mode == "last" or key in self._LAST_KEYS:
                data[key] = item[pick]
                continue
            is_bool = item.dtype == torch.bool
            if is_bool:
                item = item.int()
            normalize = key in self._NORMAL_KEYS
            if key in self._VOTING_KEYS or key in self.bins:
                if item.dim() != 1:
                    raise NotImplementedError(
                        f"'{key}': only 1-D labels are voted or binned (the reference sums 2-D "
                        "items as ready-made histograms; not built)")
                if key in self.bins:
                    out = voxel.group_histogram(item, groups, self.bins[key])
                else:
                    out = voxel.group_vote(item, groups)
                if normalize:
                    out = out / out.norm(dim=1).view(-1, 1)
            else:
                out = voxel.group_mean(item, groups, normalize=normalize)
            data[key] = out.bool() if is_bool else out
        if self.quantize_coords:
            coords = groups.coords.clone()
            if not self.allow_negative_coords:
                coords -= torch.min(coords, dim=0, keepdim=True).values
            data.coords = coords
        data.grid_size = torch.tensor([self.grid_size])
        return data


class PartitionAdjacency:
    """The three reference steps ``AdjacencyGraph(k, w)`` -> ``ConnectIsolated(k_isolated)`` ->
    ``Data.to_trimmed(reduce)`` (src/transforms/graph.py:45-96, 1455-1472, src/data/data.py:
    563-586; the last one opens ``CutPursuitPartition._process``, src/transforms/partition.py:141)
    fused into ``graph.partition_adjacency``: takes a ``Data`` with ``neighbor_index`` /
    ``neighbor_distance`` / ``pos`` (and ``batch`` if present), returns it with the trimmed,
    (i, j)-sorted ``edge_index`` / ``edge_attr`` and ``edge_source_csr`` [N + 1], the forward
    star's row pointers (``edge_index[1]`` is its target array)."""

    def __init__(self, k=10, w=-1, k_isolated=1, reduce="mean"):
        self.k, self.w, self.k_isolated, self.reduce = k, w, k_isolated, reduce

    def __call__(self, data):
        from .graph import partition_adjacency
        if data.neighbor_index is None:
            raise ValueError("PartitionAdjacency needs data.neighbor_index (run the kNN first)")
        g = partition_adjacency(data.neighbor_index, data.get("neighbor_distance"), self.k, w=self.w,
                                pos=data.get("pos"), k_isolated=self.k_isolated, reduce=self.reduce,
                                batch=data.get("batch"))
        data.edge_index, data.edge_attr, data.edge_source_csr = g.edge_index, g.edge_attr, g.source_csr
        return data


class GroundElevation:
    """``GroundElevation`` of the preprocessing chain (src/transforms/point.py:185-326,
    configs/datamodule/semantic/default.yaml between PointFeatures and AdjacencyGraph): takes a
    ``Data`` with ``pos`` [N, 3] f32 of ONE cloud on the device and returns it with
    ``elevation`` [N, 1], the height above a RANSAC ground plane divided by ``scale``
    (``ground.ground_elevation`` on ``csrc/ground.hip``).

    ``z_threshold`` / ``verticality_threshold`` / ``xy_grid`` select the reference's three
    filters; ``verticality_threshold`` needs ``data.verticality`` (``PointFeatures``).
    ``scale <= 0`` skips the transform.  ``model`` 'knn' and 'mlp' are not built.  ``kwargs``:
    ``random_state`` (seed of the hypotheses, default 0), ``residual_threshold`` (default 1e-3)
    as ``single_plane_model`` takes them, and ``num_hypotheses`` (default 100); others are
    dropped like the reference's ``filter_kwargs`` does.  The fit's record is kept as
    ``ground_plane_``."""

    _KWARGS = ("random_state", "residual_threshold", "num_hypotheses")

    def __init__(self, z_threshold=None, verticality_threshold=None, xy_grid=None, model="ransac",
                 scale=3.0, **kwargs):
        if verticality_threshold is not None:
            assert 0 < verticality_threshold < 1
        if xy_grid is not None:
            assert xy_grid > 0
        assert model in ["ransac", "knn", "mlp"]
        self.z_threshold, self.verticality_threshold, self.xy_grid = \
            z_threshold, verticality_threshold, xy_grid
        self.model, self.scale, self.kwargs = model, scale, kwargs
        self.ground_plane_ = None

    def __call__(self, data):
        from .ground import ground_elevation
        if self.scale <= 0:
            return data
        if self.model != "ransac":
            raise NotImplementedError(
                f"GroundElevation(model={self.model!r}) is not implemented: only 'ransac' is")
        verticality = None
        if self.verticality_threshold and (0 < self.verticality_threshold < 1):
            verticality = data.get("verticality")
            if verticality is None:
                raise ValueError(
                    "The Data object does not have a 'verticality' attribute. "
                    "To compute verticality, please call PointFeatures on "
                    "your Data first")
        kw = {k: v for k, v in self.kwargs.items() if k in self._KWARGS}
        elevation, plane = ground_elevation(
            data.pos, z_threshold=self.z_threshold, verticality=verticality,
            verticality_threshold=self.verticality_threshold if verticality is not None else None,
            xy_grid=self.xy_grid, scale=self.scale, **kw)
        data.elevation = elevation
        self.ground_plane_ = plane
        return data


class PointFeatures:
    """``PointFeatures`` of the preprocessing chain (src/transforms/point.py:41-182, after ``KNN``
    in configs/datamodule/semantic/default.yaml): takes a ``Data`` on the device and returns it
    with the requested keys among ``rgb`` / ``hsv`` / ``lab`` (from ``data.rgb``, uint8 in
    [0, 255] or floats in [0, 1]), ``density`` (from ``neighbor_index`` / ``neighbor_distance``)
    and the geometric keys (from ``pos`` / ``neighbor_index``); see ``features.point_features``.
    ``keys=None``: every key of the reference's ``POINT_FEATURES``.  ``chunk_size`` is accepted
    and ignored: nothing here is chunked."""

    def __init__(self, keys=None, k_min=5, k_step=-1, k_min_search=25, add_self_as_neighbor=True,
                 chunk_size=100000, overwrite=True):
        from .features import POINT_FEATURES, sanitize_keys
        self.keys = sanitize_keys(keys, default=POINT_FEATURES)
        self.k_min, self.k_step, self.k_min_search = k_min, k_step, k_min_search
        self.add_self_as_neighbor = add_self_as_neighbor
        self.chunk_size = chunk_size
        self.overwrite = overwrite

    def __call__(self, data):
        from .features import point_features
        return point_features(data, self.keys, k_min=self.k_min, k_step=self.k_step,
                              k_min_search=self.k_min_search,
                              add_self_as_neighbor=self.add_self_as_neighbor,
                              overwrite=self.overwrite)


class AddKeysTo:
    """``AddKeysTo`` (src/transforms/data.py:221-249): concatenates the attributes ``keys`` to
    the columns of ``to`` with ``Data.add_keys_to``; ``AddKeysTo(keys=partition_hf, to='x',
    delete_after=False)`` builds the ``x`` the partition reads.  ``features.partition_input``
    is this step fused with ``PointFeatures``."""

    def __init__(self, keys=None, to="x", strict=True, delete_after=True):
        self.keys = [keys] if isinstance(keys, str) else keys
        self.to, self.strict, self.delete_after = to, strict, delete_after

    def __call__(self, data):
        data.add_keys_to(keys=self.keys, to=self.to, strict=self.strict,
                         delete_after=self.delete_after)
        return data


class RemoveKeys:
    """``RemoveKeys`` (src/transforms/data.py:154-177): drops the attributes ``keys`` from a
    ``Data``; ``strict`` raises on a missing key.  The partition stage's chain ends with it
    (``edge_attr``, ``neighbor_index``, ``neighbor_distance``: the loss reads ``edge_index``
    alone)."""

    def __init__(self, keys=None, strict=False):
        from .features import sanitize_keys
        self.keys, self.strict = sanitize_keys(keys, default=()), strict

    def __call__(self, data):
        for k in self.keys:
            if k not in data and self.strict:
                raise Exception(f"key: {k} is not within Data keys: {set(data.keys)}")
        for k in self.keys:
            data[k] = None
        return data


class KNN:
    """``KNN`` (src/transforms/neighbors.py:11-88): the ``k`` nearest other points within
    ``r_max`` of every point (``neighbors.knn_1``, per cloud of a batch) into
    ``data.neighbor_index`` (-1: missing) and ``data.neighbor_distance``.  ``r_max <= 0`` or
    ``k <= 0`` skips the step.  ``save_as_csr=True`` (a ``CSRData`` of the found neighbours) is
    not built."""

    def __init__(self, k=50, r_max=1, oversample=False, self_is_neighbor=False, verbose=False,
                 save_as_csr=False):
        if save_as_csr:
            raise NotImplementedError("KNN(save_as_csr=True) is not supported: the neighbours stay "
                                      "dense [N, k] with -1 for a missing one")
        self.k, self.r_max, self.oversample = k, r_max, oversample
        self.self_is_neighbor, self.verbose, self.save_as_csr = self_is_neighbor, verbose, save_as_csr

    def __call__(self, data):
        if self.r_max <= 0 or self.k <= 0:
            return data
        from .neighbors import knn_1
        data.neighbor_index, data.neighbor_distance = knn_1(
            data.pos, self.k, r_max=self.r_max, batch=data.get("batch"), oversample=self.oversample,
            self_is_neighbor=self.self_is_neighbor)
        return data


class AdjacencyGraph:
    """``AdjacencyGraph`` (src/transforms/graph.py:45-96): the directed, untrimmed edge list
    ``(i, neighbor_index[i, j])`` for ``j < k`` in row order, without the missing (-1) neighbours,
    into ``data.edge_index``; ``data.edge_attr`` is 1 for ``w <= 0``, else
    ``1 / (w + distance / mean distance)``.  This is the graph ``criterion.PartitionCriterion``
    contrasts the features along and the partition reads its contour prior from."""

    def __init__(self, k=10, w=-1):
        self.k, self.w = k, w

    def __call__(self, data):
        nn = data.get("neighbor_index")
        assert nn is not None, \
            "Data must have 'neighbor_index' attribute to allow adjacency graph construction."
        assert data.get("neighbor_distance") is not None or self.w <= 0, \
            "Data must have 'neighbor_distance' attribute to allow adjacency graph construction."
        assert self.k <= nn.shape[1]
        source = torch.arange(nn.shape[0], device=nn.device).repeat_interleave(self.k)
        target = nn[:, :self.k].flatten()
        mask = target >= 0
        source, target = source[mask], target[mask]
        data.edge_index = torch.stack((source, target))
        if self.w > 0:
            distances = data.neighbor_distance[:, :self.k].flatten()[mask]
            data.edge_attr = 1 / (self.w + distances / distances.mean())
        else:
            data.edge_attr = torch.ones_like(source, dtype=torch.float)
        return data


class NAGRemoveKeys:
    """``NAGRemoveKeys`` (src/transforms/data.py:154-218): drops the attributes ``keys`` from the
    levels ``level`` names (an int, 'all', 'i+', 'i-'); ``strict`` raises on a missing key."""

    def __init__(self, level="all", keys=None, strict=False):
        from .features import sanitize_keys
        assert isinstance(level, (int, str))
        self.level, self.keys, self.strict = level, sanitize_keys(keys, default=()), strict

    def __call__(self, nag):
        for data, keys in zip(nag, _per_level(self.level, (), self.keys, nag.num_levels)):
            for k in keys:
                if k not in data and self.strict:
                    raise Exception(f"key: {k} is not within Data keys: {set(data.keys)}")
            for k in keys:
                data[k] = None
        return nag


class SegmentFeatures:
    """``SegmentFeatures`` (src/transforms/graph.py:117-321): the handcrafted features of every
    level above 0 from the level-0 points, written into the level's attributes under the
    reference's names (``<key>``, ``mean_<key>``, ``std_<key>``) by ``segment.segment_features``.
    ``strict`` raises when a ``mean_keys`` / ``std_keys`` entry is no level-0 attribute; otherwise
    the entry is skipped.  The sample of ``n_min`` .. ``n_max`` points per segment is drawn from
    torch's generator (``torch.manual_seed``)."""

    def __init__(self, n_max=32, n_min=5, keys=None, mean_keys=None, std_keys=None, strict=True):
        from .features import POINT_FEATURES, sanitize_keys
        from .segment import SEGMENT_BASE_FEATURES
        self.n_max, self.n_min = n_max, n_min
        self.keys = sanitize_keys(keys, default=SEGMENT_BASE_FEATURES)
        self.mean_keys = sanitize_keys(mean_keys, default=POINT_FEATURES)
        self.std_keys = sanitize_keys(std_keys, default=POINT_FEATURES)
        self.strict = strict

    def __call__(self, nag):
        from .segment import segment_features
        atoms = nag[0]
        for what, keys in (("mean", self.mean_keys), ("std", self.std_keys)):
            for key in keys:
                if atoms.get(key) is None and self.strict:
                    raise ValueError(f"No point key `{key}` to build '{what}_{key} key'")
        mean_keys = [k for k in self.mean_keys if atoms.get(k) is not None]
        std_keys = [k for k in self.std_keys if atoms.get(k) is not None]
        attrs = {k: atoms[k] for k in set(mean_keys) | set(std_keys)}
        for i in range(1, nag.num_levels):
            data = nag[i]
            out = segment_features(atoms.pos, nag.get_super_index(i), data.num_nodes,
                                   sub_size=nag.get_sub_size(i, low=0), n_max=self.n_max,
                                   n_min=self.n_min, keys=self.keys, mean_keys=mean_keys,
                                   std_keys=std_keys, point_attrs=attrs)
            for k, v in out.items():
                data[k] = v
        return nag


class RadiusHorizontalGraph:
    """``RadiusHorizontalGraph`` (src/transforms/graph.py:594-947): for every level above 0 the
    graph of segments with points ``gap`` or less apart (``cluster_radius_nn_graph`` with at most
    ``k_max`` neighbours), every node without an edge linked to its ``k_min`` nearest nodes
    (``graph.connect_isolated``), trimmed, with the 7 stored edge features in ``edge_attr``
    (``graph.superedge_features`` on ``csrc/superedge.hip``: the anchors of a level's final edge
    list are searched once, not per chunk).  ``k_min``, ``k_max``, ``gap``, ``se_ratio``, ``se_min``,
    ``cycles`` and ``margin`` may be lists, one entry per level above 0.  ``pca_on_cpu``,
    ``chunk_size`` and ``verbose`` are accepted and ignored.  ``keys`` must hold 'mean_off',
    'std_off' and 'mean_dist': all three are stored, as in the reference."""

    def __init__(self, k_min=1, k_max=100, gap=0, se_ratio=0.2, se_min=20, cycles=3,
                 pca_on_cpu=False, margin=0.2, chunk_size=100000, halfspace_filter=True,
                 bbox_filter=True, target_pc_flip=True, source_pc_sort=False, keys=None,
                 verbose=False):
        from .features import sanitize_keys
        if isinstance(k_min, list):
            assert all([k > 0 for k in k_min]), \
                "k_min must be 1 or more, to avoid any unpleasant downstream " \
                "issues where nodes have no edge"
        else:
            assert k_min > 0, \
                "k_min must be 1 or more, to avoid any unpleasant downstream " \
                "issues where nodes have no edge"
        self.k_min, self.k_max, self.gap = k_min, k_max, gap
        self.se_ratio, self.se_min, self.cycles, self.margin = se_ratio, se_min, cycles, margin
        self.pca_on_cpu, self.chunk_size, self.verbose = pca_on_cpu, chunk_size, verbose
        self.halfspace_filter, self.bbox_filter = halfspace_filter, bbox_filter
        self.target_pc_flip, self.source_pc_sort = target_pc_flip, source_pc_sort
        self.keys = sanitize_keys(keys, default=("mean_off", "std_off", "mean_dist"))

    def __call__(self, nag):
        from .graph import connect_isolated, superedge_features, to_trimmed
        from .neighbors import cluster_radius_nn_graph
        if not all(k in self.keys for k in ("mean_off", "std_off", "mean_dist")):
            raise NotImplementedError(
                "For now, 'mean_off', 'std_off' and 'mean_dist' must all be computed, since we "
                "must store them all into 'edge_attr'.")
        n = nag.num_levels - 1

        def per_level(v):
            return list(v) if isinstance(v, list) else [v] * n
        params = zip(range(1, nag.num_levels), *(per_level(v) for v in (
            self.k_min, self.k_max, self.gap, self.se_ratio, self.se_min, self.cycles, self.margin)))
        for i, k_min, k_max, gap, ratio, se_min, cycles, margin in params:
            data = nag[i]
            num_nodes = data.num_nodes
            data.edge_index = None
            data.edge_attr = None
            if num_nodes < 2:
                raise ValueError(f"Input NAG only has 1 node at level={i}. Cannot compute "
                                 f"radius-based horizontal graph.")
            if data.edge_keys:
                raise NotImplementedError(f"edge keys {data.edge_keys} are not carried through the "
                                          "horizontal graph")
            super_index = nag.get_super_index(i)
            edge_index, _ = cluster_radius_nn_graph(
                nag[0].pos, super_index, k_max=k_max, gap=gap, batch=data.batch, trim=True,
                cycles=cycles, num_clusters=num_nodes)
            edge_index = connect_isolated(edge_index, data.pos, k_min, batch=data.batch,
                                          num_nodes=num_nodes)
            edge_index = to_trimmed(edge_index)
            data.edge_index, data.edge_attr = superedge_features(
                nag[0].pos, super_index, edge_index, ratio=ratio, k_min=se_min, cycles=cycles,
                margin=margin, halfspace_filter=self.halfspace_filter,
                bbox_filter=self.bbox_filter, target_pc_flip=self.target_pc_flip,
                source_pc_sort=self.source_pc_sort, num_segments=num_nodes)
        return nag


class GreedyContourPriorPartition:
    """``GreedyContourPriorPartition`` (src/transforms/partition.py:383-653): a hierarchical
    partition by greedy merges on the contour-prior energy, one level per entry of ``min_size`` /
    ``reg`` (a scalar is repeated), on ``partition.merge_components_by_contour_prior_on_data``
    (``csrc/merge.hip`` for CUDA tensors).  Takes a ``Data`` with ``pos``, ``x``, ``edge_index``
    and returns a ``NAG``: level ``l`` gains ``super_index``, level ``l + 1`` carries ``pos``,
    ``node_size``, ``sub``, ``x``, ``edge_index``, ``edge_attr`` and the int64 sums of ``y`` /
    ``semantic_pred`` histograms when present.  As in the reference every level recomputes
    ``edge_attr`` from ``edge_weight_mode`` (so 'unit' resets merged weights to one) and
    ``spatial_weight`` appends ``spatial_weight * pos`` to ``x`` at every level.  Weights are f32
    (the reference's 'unit' mode makes int64 ones).  ``sharding`` and ``verbose`` are accepted
    and ignored.  Refused: ``k > 0`` and the two 'affinity' weight modes."""

    def __init__(self, reg, min_size, spatial_weight=None, edge_weight_mode='unit', d_0=None,
                 edge_reduce='add', k=0, w_adjacency=0, max_iterations=-1, verbose=False,
                 sharding=None):
        from .partition import EDGE_WEIGHT_MODES, REDUCES, check_edge_weight_mode
        self.spatial_weight, self.edge_weight_mode, self.d_0 = spatial_weight, edge_weight_mode, d_0
        self.edge_reduce, self.k, self.w_adjacency = edge_reduce, k, w_adjacency
        self.max_iterations, self.verbose, self.sharding = max_iterations, verbose, sharding
        assert edge_weight_mode in EDGE_WEIGHT_MODES, \
            (f"Invalid edge weight mode: {edge_weight_mode}.\n"
             f"Valid options are: {list(EDGE_WEIGHT_MODES)}")
        check_edge_weight_mode(edge_weight_mode)
        if k > 0:
            raise NotImplementedError(
                "k > 0 (reconnecting isolated components every round) is not built")
        if edge_reduce not in REDUCES:
            raise ValueError(f"edge_reduce must be one of {sorted(REDUCES)}, got {edge_reduce!r}")

        def is_list(v):
            return isinstance(v, (list, tuple))
        if is_list(min_size):
            num_levels = len(min_size)
        elif is_list(reg):
            num_levels = len(reg)
        else:
            num_levels = 1
        assert isinstance(reg, (int, float)) or is_list(reg), \
            "`reg` parameter expected a scalar or a List"
        self.reg = list(reg) if is_list(reg) else [reg] * num_levels
        assert isinstance(min_size, int) or is_list(min_size), \
            "`min_size` parameter expected an int or a List"
        self.min_size = list(min_size) if is_list(min_size) else [min_size] * num_levels
        assert len(self.reg) == len(self.min_size), \
            "Expected the same number of `reg` and `min_size` parameters"

    def __call__(self, data):
        from .data import Data, NAG
        from .partition import edge_weights, merge_components_by_contour_prior_on_data
        data_list = [data]
        for level, (reg, min_size) in enumerate(zip(self.reg, self.min_size)):
            d1 = data_list[level]
            if d1.x is None or d1.pos is None or d1.edge_index is None:
                raise ValueError("GreedyContourPriorPartition needs data.x, data.pos and data.edge_index")
            d1.edge_attr = edge_weights(d1.pos, d1.x, d1.edge_index, self.edge_weight_mode, self.d_0)
            if self.spatial_weight is not None and self.spatial_weight != 0:
                x = d1.x if d1.x.dim() > 1 else d1.x.view(-1, 1)
                d1.x = torch.cat([x, d1.pos * self.spatial_weight], dim=1)
            d1, (X_merged, S_merged, E_cp, W_cp, P_merged, sub) = \
                merge_components_by_contour_prior_on_data(
                    d1, reg, min_size, False, self.k, self.w_adjacency, self.max_iterations,
                    self.sharding, self.edge_reduce, self.verbose)
            data_list[level] = d1
            d2 = Data(pos=P_merged, node_size=S_merged, sub=sub, x=X_merged, edge_index=E_cp,
                      edge_attr=W_cp)
            for key in ('y', 'semantic_pred'):
                if key not in d1:
                    continue
                hist = d1[key]
                assert hist.dim() == 2, \
                    f"Expected Data.{key} to hold `(num_nodes, num_classes)` histograms, not single labels"
                if hist.is_cuda:
                    from .ops import segment_sum_i64
                    d2[key] = segment_sum_i64(hist.long(), d1.super_index, S_merged.numel())
                else:
                    d2[key] = torch.zeros((S_merged.numel(), hist.shape[1]), dtype=torch.int64) \
                        .index_add_(0, d1.super_index, hist.long())
            data_list.append(d2)
        return NAG(data_list)


# ---------------------------------------------------------------------------
# Per-batch on-device transforms of the training pipeline
# (configs/datamodule/semantic/default.yaml:206-290), on the NAG mirror of data.py
# ---------------------------------------------------------------------------


class NodeSize:
    """``node_size`` of every level above ``low`` = number of ``low``-level nodes it
    holds (src/transforms/graph.py:1475-1498)."""

    def __init__(self, low=0):
        self.low = low

    def __call__(self, nag):
        for i in range(self.low + 1, nag.num_levels):
            nag[i].node_size = nag.get_sub_size(i, low=self.low)
        return nag


class SampleSubNodes:
    """Keep ``n_min``..``n_max`` random ``low``-level nodes of every ``high``-level
    segment (src/transforms/sampling.py:656-715)."""

    def __init__(self, high=1, low=0, n_max=32, n_min=16, mask=None, seed=None):
        self.high, self.low, self.n_max, self.n_min, self.mask, self.seed = \
            high, low, n_max, n_min, mask, seed

    def __call__(self, nag):
        if self.low == self.high:
            return nag
        idx = nag.get_sampling(high=self.high, low=self.low, n_max=self.n_max, n_min=self.n_min,
                               mask=self.mask, return_pointers=False, seed=self.seed)
        return nag.select(self.low, idx)


def segment_sampling_weights(nag, i_level, by_size=False, by_class=False):
    """Probability of drawing each level-``i_level`` segment (sampling.py:771-798 and
    895-921, the same lines twice): uniform, plus - ``by_size`` - the cube root of the number
    of points it holds, plus - ``by_class`` - the rarity of the rarest class it contains
    (``y`` = per-segment label histogram), each term normalised to sum 1 before it is added."""
    data = nag[i_level]
    w = torch.ones(data.num_nodes, device=nag.device)
    if by_size:
        sw = nag.get_sub_size(i_level, low=0) ** 0.333
        w = w + sw / sw.sum()
    if by_class and "y" in data:
        scores = 1 / (data.y.sum(dim=0).sqrt() + 1)
        scores = scores / scores.sum()
        cw = (data.y.gt(0) * scores.view(1, -1)).max(dim=1).values
        w = w + (cw / cw.sum()).squeeze()
    return w / w.sum()


class SampleSegments:
    """Drop a ``ratio`` of the segments of every level >= 1, from the top level down
    (src/transforms/sampling.py:718-807)."""

    def __init__(self, ratio=0.2, by_size=False, by_class=False):
        assert isinstance(ratio, list) and all(0 <= r < 1 for r in ratio) or (0 <= ratio < 1)
        self.ratio, self.by_size, self.by_class = ratio, by_size, by_class

    def __call__(self, nag):
        L = nag.num_levels
        ratio = self.ratio if isinstance(self.ratio, list) else [self.ratio] * (L - 1)
        for i in range(L - 1, 0, -1):
            if ratio[i - 1] <= 0:
                continue
            n = nag[i].num_nodes
            keep = n - int(n * ratio[i - 1])
            w = segment_sampling_weights(nag, i, self.by_size, self.by_class)
            idx = torch.multinomial(w, keep, replacement=False)
            nag = nag.select(i, idx)
        return nag


class SampleEdges:
    """Keep ``n_min``..``n_max`` random outgoing edges per source node
    (src/transforms/sampling.py:1234-1312) on the levels ``levels``."""

    def __init__(self, levels=(1, 2), n_min=16, n_max=32, seed=None):
        self.levels, self.n_min, self.n_max, self.seed = tuple(levels), n_min, n_max, seed

    def __call__(self, nag):
        from .segment import sparse_sample
        for i in self.levels:
            if i >= nag.num_levels or self.n_min < 0 or self.n_max < 0:
                continue
            d = nag[i]
            if not d.has_edges:
                continue
            idx = sparse_sample(d.edge_index[0], n_max=self.n_max, n_min=self.n_min,
                                seed=self.seed, num_segments=d.num_nodes)
            d.edge_index = d.edge_index[:, idx]
            for key in ["edge_attr"] + d.edge_keys:
                if key in d:
                    d[key] = d[key][idx]
        return nag


class OnTheFlyHorizontalEdgeFeatures:
    """18-D edge features from the stored 7-D ones + node attributes, edges doubled, and
    (``add_self_loops``) ``NAGAddSelfLoops`` fused (src/transforms/graph.py:1063-1277,
    1419-1452)."""

    def __init__(self, add_self_loops=True, use_mean_normal=False):
        self.add_self_loops = add_self_loops
        self.normal_key = "mean_normal" if use_mean_normal else "normal"

    def __call__(self, nag):
        for i in range(1, nag.num_levels):
            d = nag[i]
            if not d.has_edges:
                continue
            d.edge_index, d.edge_attr = horizontal_edge_features(
                d.edge_index, d.edge_attr, d.pos, d[self.normal_key], d.log_length, d.log_surface,
                d.log_volume, d.log_size, add_self_loops=self.add_self_loops)
        return nag


class SampleRadiusSubgraphs:
    """Keep the level-``i_level`` nodes within ``r`` of ``k`` random seed nodes (at most
    the ``k_max`` nearest per seed), each neighbourhood as its own batch item when
    ``disjoint`` (src/transforms/sampling.py:810-1000, 1094-1230).  Seeds are drawn like
    the reference (``torch.multinomial`` over ``segment_sampling_weights``, spread over the
    batch items when the level carries a ``batch``); ``idx_seed`` overrides the draw."""

    def __init__(self, r=2, k_max=10000, i_level=1, k=1, use_batch=True, disjoint=False,
                 cylindrical=False, idx_seed=None, by_size=False, by_class=False):
        self.r, self.k_max, self.i_level, self.k = r, k_max, i_level, k
        self.use_batch, self.disjoint, self.cylindrical, self.idx_seed = \
            use_batch, disjoint, cylindrical, idx_seed
        self.by_size, self.by_class = by_size, by_class

    def _seeds(self, data, k, w):
        batch = data.batch if "batch" in data else None
        if batch is None or not self.use_batch:
            return torch.multinomial(w, k, replacement=False)
        ids = batch.unique()
        ids = ids[torch.randperm(ids.numel())]
        kb = max(k // ids.numel(), 1)
        out, done = [], 0
        for step, b in enumerate(ids):
            if step >= ids.numel() - 1:
                kb = k - done
            m = torch.where(batch == b)[0]
            out.append(m[torch.multinomial(w[m], kb, replacement=False)])
            done += kb
            if done >= k:
                break
        return torch.cat(out)

    def _ball(self, data, seed):
        from .ops import _workspace
        dev = data.device
        pos = data.pos.detach().float().contiguous()
        n = pos.shape[0]
        batch = data.batch.long().contiguous() if "batch" in data else None
        c = pos[seed].cpu()
        center = (ctypes.c_float * 3)(float(c[0]), float(c[1]), float(c[2]))
        out = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        nbytes = _lib.lib.spt_radius_ball_workspace_bytes(n)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_radius_ball_f32(
                _lib.ptr(pos), n, ctypes.cast(center, ctypes.c_void_p), float(self.r),
                int(self.cylindrical), _lib.ptr(batch), int(batch[seed]) if batch is not None else 0,
                _lib.ptr(out), _lib.ptr(count), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_radius_ball_f32")
        idx = out[:int(count)]
        if idx.numel() > self.k_max:                      # keep the k_max nearest (rare)
            w = torch.tensor([1.0, 1.0, 0.0 if self.cylindrical else 1.0], device=dev)
            d = ((pos[idx] - pos[seed]) * w).norm(dim=1)
            idx = idx[torch.topk(d, self.k_max, largest=False).indices].sort().values
        return idx

    def __call__(self, nag):
        from .data import NAG
        if self.i_level is None or self.k <= 0 or self.r is None or self.r <= 0:
            return nag
        i_level = nag.num_levels - 1 if self.i_level == -1 else self.i_level
        data = nag[i_level]
        k = self.k if self.k < data.num_nodes else 1
        seeds = self.idx_seed if self.idx_seed is not None else self._seeds(
            data, k, segment_sampling_weights(nag, i_level, self.by_size, self.by_class))
        balls = [self._ball(data, int(s)) for s in seeds]
        if self.disjoint:
            return NAG.from_nag_list([nag.select(i_level, idx) for idx in balls])
        return nag.select(i_level, torch.unique(torch.cat(balls)))


def _per_level(level, default, value, num_levels, start=0):
    """``fill_list_with_string_indexing`` (src/utils/list.py:46-91): ``value`` on the levels
    ``level`` names - an int, 'all', 'i+' (level i and above) or 'i-' (the levels BELOW i) - and
    ``default`` elsewhere."""
    out = [default] * num_levels
    if isinstance(level, int):
        out[level] = value
    elif level == "all":
        out[start:] = [value] * (num_levels - start)
    elif level[-1] == "+":
        i = int(level[:-1])
        out[i:] = [value] * (num_levels - i)
    elif level[-1] == "-":
        i = int(level[:-1])
        out[:i] = [value] * i
    else:
        raise ValueError(f"Unsupported level={level}")
    return out


class NAGRestrictSize:
    """Cap the number of nodes and / or edges of the levels ``level`` by uniform random removal
    (src/transforms/sampling.py:1346-1423; in the training pipeline after the samplers, with
    ``level='1+'``): surplus nodes go through ``NAG.select`` (their descendants and ancestors
    follow), surplus edges are dropped with their attributes."""

    def __init__(self, level="1+", num_nodes=0, num_edges=0):
        self.level, self.num_nodes, self.num_edges = level, num_nodes, num_edges

    def __call__(self, nag):
        L = nag.num_levels
        nodes = _per_level(self.level, -1, self.num_nodes, L)
        edges = _per_level(self.level, -1, self.num_edges, L)
        for i in range(L):
            nag = self._restrict_level(nag, i, nodes[i], edges[i])
        return nag

    @staticmethod
    def _restrict_level(nag, i_level, num_nodes, num_edges):
        d = nag[i_level]
        if d.num_nodes > num_nodes and num_nodes > 0:
            idx = torch.multinomial(torch.ones(d.num_nodes, device=nag.device), num_nodes,
                                    replacement=False)
            nag = nag.select(i_level, idx)
            d = nag[i_level]
        if d.num_edges > num_edges and num_edges > 0:
            idx = torch.multinomial(torch.ones(d.num_edges, device=nag.device), num_edges,
                                    replacement=False)
            keys = [k for k in ["edge_attr"] + d.edge_keys if k in d]      # before the cut
            d.edge_index = d.edge_index[:, idx]
            for key in keys:
                d[key] = d[key][idx]
        return nag


class OnTheFlyInstanceGraph:
    """Targets of the panoptic heads, built every batch (src/transforms/instance.py:18-257):
    the trimmed graph between the level-``level`` segments (``obj_edge_index``: the existing
    edges, or segments with points / centroids within ``radius``), the affinity of each edge
    from the segments' overlaps with the annotated objects (``obj_edge_affinity``,
    ``InstanceData.instance_graph``) and the position of each segment's target object
    (``obj_pos``)."""

    _ADJACENCY_MODES = ["available", "radius-atomic", "radius-centroid"]
    _CENTROID_MODES = ["iou", "ratio-product"]

    def __init__(self, level=1, num_classes=None, adjacency_mode="radius-atomic", k_max=30,
                 radius=1, use_batch=True, centroid_mode="iou", centroid_level=1,
                 smooth_affinity=True):
        assert adjacency_mode.lower() in self._ADJACENCY_MODES, \
            f"Expected 'mode' to be one of {self._ADJACENCY_MODES}"
        assert centroid_mode.lower() in self._CENTROID_MODES, \
            f"Expected 'mode' to be one of {self._CENTROID_MODES}"
        self.level, self.num_classes = level, num_classes
        self.adjacency_mode, self.k_max, self.radius = adjacency_mode.lower(), k_max, radius
        self.use_batch, self.centroid_mode = use_batch, centroid_mode.lower()
        self.centroid_level, self.smooth_affinity = centroid_level, smooth_affinity

    def __call__(self, nag):
        from .graph import to_trimmed
        from .instance import _consecutive
        from .neighbors import cluster_radius_nn_graph, knn_1_graph
        if self.level is None or self.level < 0:
            return nag
        if not 0 <= self.level < nag.num_levels:
            raise AssertionError(f"level {self.level} is not in the NAG")
        data = nag[self.level]
        batch = data.batch if (self.use_batch and "batch" in data) else None
        if self.adjacency_mode == "available":
            obj_edge_index = data.edge_index if data.has_edges else None
        elif self.adjacency_mode == "radius-atomic":
            obj_edge_index, _ = cluster_radius_nn_graph(
                nag[0].pos, nag.get_super_index(self.level, low=0), k_max=self.k_max,
                gap=self.radius, batch=batch)
        else:
            obj_edge_index, _ = knn_1_graph(data.pos, self.k_max, r_max=self.radius, batch=batch)
        if obj_edge_index is None:
            obj_edge_index = torch.empty(2, 0, dtype=torch.long, device=data.device)

        if "obj" not in data:                               # no annotations: graph only
            data.obj_edge_index = to_trimmed(obj_edge_index)
            data.obj_edge_affinity = None
            data.obj_pos = None
            return nag

        data.obj_edge_index, data.obj_edge_affinity = data.obj.instance_graph(
            obj_edge_index, num_classes=self.num_classes, smooth_affinity=self.smooth_affinity)

        # position of each segment's target object: objects' centroids estimated at
        # ``centroid_level``, looked up through a common dense numbering of the object ids
        i_level = min(self.centroid_level, nag.num_levels - 1)
        # 'ratio-product' is the transform's name (transforms/instance.py:101-119) for what
        # InstanceData.estimate_centroid implements as 'product-iou' (data/instance.py:337): the
        # reference forwards the string unchanged and raises there; it is mapped here
        mode = "product-iou" if self.centroid_mode == "ratio-product" else self.centroid_mode
        obj_pos, obj_idx = nag[i_level].estimate_instance_centroid(mode=mode)
        sp_obj_idx = data.obj.major(num_classes=self.num_classes)[0]
        joint = torch.cat((sp_obj_idx, obj_idx))
        dense = _consecutive(joint)[0]
        data.obj_pos = obj_pos[dense[:sp_obj_idx.numel()]]
        return nag


def morton_code(pos, bits=10):
    """``bits``-per-axis Morton (Z-order) code of [n, 3] positions inside their bounding box (int64)."""
    lo, hi = pos.min(0).values, pos.max(0).values
    top = (1 << bits) - 1
    q = ((pos - lo) / (hi - lo).clamp_min(1e-9) * float(top)).long().clamp_(0, top)
    code = torch.zeros(pos.shape[0], dtype=torch.int64, device=pos.device)
    for b in range(bits):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return code


class MortonOrder:
    """Load-time re-ordering of a NAG for MEMORY LOCALITY (round 5; not a transform of the
    reference - its datasets store nodes in the order the partition emitted them, spatial neighbours
    ~0.23 N apart in the demo room).  The top level is sorted by (cloud, Morton code of its
    position); every level below is sorted by its parent (in the parent's new numbering) and,
    inside a parent, by its own Morton code - each step one ``NAG.select`` with a permutation
    (src/data/nag.py:306-399), which re-indexes edges, ``super_index`` and ``sub`` consistently.  Afterwards the nodes a superpoint-graph edge
    joins (built by radius search, src/transforms/graph.py:193-321: spatial neighbours) are close
    in memory at every level, the children of a superpoint are contiguous (the pool's CSR view is
    the identity: coalesced streams instead of gathers), and the attention's k / v / record gathers
    hit rows that are still in L2.

    Purely a renumbering: edges, ``super_index``, ``sub`` and every per-node attribute follow.
    ``nag[i].morton_origin`` [n_i] = the ORIGINAL index of every node, so per-node outputs go
    back with ``MortonOrder.restore`` (``out_original[origin] = out``); results are those of the
    un-ordered NAG up to the summation order of segment / attention reductions."""

    KEY = "morton_origin"

    def __init__(self, bits=10):
        self.bits = int(bits)

    def __call__(self, nag):
        nag = nag.clone()
        L = nag.num_levels
        for i in range(L):
            n = nag[i].num_nodes
            nag[i][self.KEY] = torch.arange(n, device=nag.device)
        top = L - 1
        d = nag[top]
        key = morton_code(d.pos, self.bits)
        if d.batch is not None:
            key = key + (d.batch.long() << (3 * self.bits))
        nag = nag.select(top, torch.argsort(key, stable=True))
        # (NAG.select re-indexes the levels below a re-ordered level but leaves their nodes where
        # they are: every level is sorted explicitly - by parent, then by its own Morton code;
        # the points of level 0 by parent only, in their stored order)
        for i in range(top - 1, -1, -1):
            d = nag[i]
            key = d.super_index.long() << (3 * self.bits)
            if i > 0:
                key = key + morton_code(d.pos, self.bits)
            nag = nag.select(i, torch.argsort(key, stable=True))
        return nag

    @classmethod
    def restore(cls, nag, out, i_level):
        """Per-node tensor ``out`` [n_i, ...] of the re-ordered level ``i_level`` back in the
        original node order."""
        origin = nag[i_level][cls.KEY]
        back = torch.empty_like(out)
        back[origin] = out
        return back


# ---------------------------------------------------------------------------
# Augmentations of the training chain (configs/datamodule/semantic/default.yaml:250-264 and
# 292-358), kernels in csrc/augment.hip, wrappers in augment.py.
#
# Every class is the reference's class of that name with its constructor signature, split in
#   draw(nag)  -> params   host only: torch's CPU generator, in the order each docstring gives
#   apply(nag, params)     no host read of device memory
# and __call__ = apply(nag, draw(nag)).  A scalar decision (rotation, scale, flip, dropped
# columns, contrast, blend, drop) is a host value in `params`; a per-element or per-row draw is
# a 64-bit seed (segment._draw_seed: one torch.randint on the CPU generator) of the counter-based
# generator, so torch.manual_seed makes a chain reproducible.
# ---------------------------------------------------------------------------
_NORMAL_KEYS = ("normal", "mean_normal")


def _f32(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (run NAGCast first), got {t.dtype}")
    return t


def _as_level_list(v, num_levels):
    return list(v) if isinstance(v, list) else [v] * num_levels


def _geometry_apply(nag, jitter=None, tilt=None, scale=None, flip=None):
    """The geometric steps that are not None / skipped, fused: one launch per tensor touched.
    ``jitter`` = {level: (sigma, trunc, seed)} of ``pos``, ``tilt`` = {'skip', 'R'}, ``scale`` =
    {'scale'}, ``flip`` = {'flip', 'axis'}."""
    from . import augment as A
    R = None if tilt is None or tilt["skip"] else tilt["R"]
    s = None if scale is None else scale["scale"]
    axis = None if flip is None or not flip["flip"] else flip["axis"]
    for i in range(nag.num_levels):
        d = nag[i]
        jit = None if jitter is None else jitter.get(i)
        if d.pos is not None and (jit is not None or R is not None or s is not None
                                  or axis is not None):
            A.geometry_(_f32(d.pos, "pos"), A.POS, jitter=jit, R=R, scale=s, flip_axis=axis)
        if R is None and s is None and axis is None:
            continue
        for k in _NORMAL_KEYS:
            t = d.get(k)
            if t is not None:
                A.geometry_(_f32(t, k), A.NORMAL, R=R, scale=s, flip_axis=axis)
        ea = d.edge_attr
        if ea is not None:
            assert ea.shape[1] == 7, \
                "Expected exactly 7 features in `edge_attr`, generated with " \
                "`_minimalistic_horizontal_edge_features`"
            A.geometry_(_f32(ea, "edge_attr"), A.EDGE7, R=R, scale=s, flip_axis=axis)
    return nag


class NAGJitterKey:
    """``NAGJitterKey`` (src/transforms/data.py:651-721): ``nag[i][key] += noise`` in place, noise
    from the truncated normal of ``torch.nn.init.trunc_normal_(std=sigma, a=-trunc, b=trunc)``
    (``trunc <= 0``: untruncated; one generator here, its tail ends at 5.42 sigma - see
    ``augment``).  ``sigma`` / ``trunc`` may be per-level lists; ``sigma <= 0`` skips the level; a
    missing key is skipped, or raises ``ValueError`` when ``strict``.

    ``draw``: one ``segment._draw_seed()`` per (level, key) that is jittered, levels in order,
    keys in order inside a level."""

    def __init__(self, key=None, sigma=0.01, trunc=0.05, strict=False):
        assert key is not None, "A key or list of keys must be specified"
        assert isinstance(sigma, (int, float, list))
        assert isinstance(trunc, (int, float, list))
        self.key = [key] if isinstance(key, str) else list(key)
        self.sigma, self.trunc, self.strict = sigma, trunc, strict

    def draw(self, nag):
        from .segment import _draw_seed
        L = nag.num_levels
        sigma, trunc = _as_level_list(self.sigma, L), _as_level_list(self.trunc, L)
        params = {}
        for i in range(L):
            if sigma[i] <= 0:
                continue
            for k in self.key:
                if nag[i].get(k) is None:
                    if self.strict:
                        raise ValueError(f"Input data does not have any '{k} attribute")
                    continue
                params[(i, k)] = (float(sigma[i]), float(trunc[i]), _draw_seed())
        return params

    def apply(self, nag, params):
        from . import augment as A
        for (i, k), (sigma, trunc, seed) in params.items():
            A.jitter_(_f32(nag[i][k], k), sigma, trunc, seed=seed)
        return nag

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class RandomTiltAndRotate:
    """``RandomTiltAndRotate`` (src/transforms/geometry.py:28-115): rotates ``pos``, ``normal``,
    ``mean_normal`` (rows with z < 0 negated afterwards) and columns 0:3 of a 7-column
    ``edge_attr`` (another width raises ``AssertionError``) of every level by ONE random matrix.

    What the reference does, where it differs from its docstring: the axis offset is
    ``MultivariateNormal(0, eye(2) * sigma)`` whose second positional argument is the COVARIANCE
    (geometry.py:66-69), so the per-axis standard deviation is ``sqrt(sigma)`` with
    ``sigma = phi / 180 * pi / 3``; ``phi == 0`` skips every level whatever ``theta`` is
    (geometry.py:86-87).  ``R`` is ``rodrigues_rotation_matrix`` (src/utils/geometry.py:27-39)
    evaluated on the host in f32 with the same torch operations.

    ``draw``: the ``MultivariateNormal.sample()`` of two values (only when ``phi > 0``), then
    ``torch.rand(1)`` for the angle (always, as the reference)."""

    def __init__(self, phi=5, theta=180):
        assert isinstance(phi, (int, float))
        assert isinstance(theta, (int, float))
        self.phi, self.theta = float(abs(phi)), float(abs(theta))

    @staticmethod
    def rotation_matrix(axis, theta_degrees):
        """``rodrigues_rotation_matrix`` on host f32 tensors, operation for operation."""
        import numpy as np
        axis = axis / axis.norm()
        k = axis
        K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        t = torch.tensor([theta_degrees / 180. * np.pi])
        return torch.eye(3) + torch.sin(t) * K + (1 - torch.cos(t)) * K.mm(K)

    def draw(self, nag=None):
        sigma = self.phi / 180. * torch.pi / 3
        if sigma > 0:
            dist = torch.distributions.MultivariateNormal(torch.zeros(2), torch.eye(2) * sigma)
            axis = torch.cat((dist.sample(), torch.ones(1)))
            axis /= axis.norm()
        else:
            axis = torch.zeros(3, dtype=torch.float)
            axis[2] = 1
        theta = torch.rand(1) * 2 * self.theta - self.theta
        return {"skip": sigma <= 0, "R": self.rotation_matrix(axis, theta)}

    def apply(self, nag, params):
        return _geometry_apply(nag, tilt=params)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class RandomAnisotropicScale:
    """``RandomAnisotropicScale`` (src/transforms/geometry.py:118-186): ``pos * scale``, normals
    ``F.normalize(normal * scale)``, ``edge_attr[:, :3] * scale`` and ``edge_attr[:, 3:] *
    ||scale||_2`` (7 columns, another width raises).  Despite the name ONE uniform draw is shared
    by the three axes: ``scale = 1 + (torch.rand(1) * 2 * delta - delta)`` (geometry.py:159), so
    the axes differ only when ``delta`` is a 3-list.

    ``draw``: ``torch.rand(1)``."""

    def __init__(self, delta=0.2):
        assert isinstance(delta, (float, int)) or isinstance(delta, (tuple, list))
        if isinstance(delta, (float, int)):
            delta = [float(delta)] * 3
        assert len(delta) == 3
        self.delta = torch.tensor(delta).abs().view(1, -1)

    def draw(self, nag=None):
        scale = 1 + (torch.rand(1) * 2 * self.delta - self.delta)
        return {"scale": scale.view(3).float()}

    def apply(self, nag, params):
        return _geometry_apply(nag, scale=params)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class RandomAxisFlip:
    """``RandomAxisFlip`` (src/transforms/geometry.py:189-245): negates column ``axis`` of
    ``pos``, of the normals (rows with z < 0 negated afterwards) and of a 7-column ``edge_attr``.
    The flip happens when the draw is ``<= p``: the reference returns early on ``rand > p``
    (geometry.py:215).

    ``draw``: ``torch.rand(1)``."""

    def __init__(self, axis=0, p=0.5):
        assert isinstance(axis, int)
        assert isinstance(p, float)
        self.axis, self.p = axis, p

    def draw(self, nag=None):
        return {"flip": not bool(torch.rand(1) > self.p), "axis": self.axis}

    def apply(self, nag, params):
        return _geometry_apply(nag, flip=params)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


def _dropout_apply(nag, columns=None, rows=None, jitter=None, inplace=True, to_mean=False):
    """Jitter, column dropout and row dropout of every (level, key) named by the three parameter
    dicts, one launch per tensor.  ``to_mean`` takes a torch composition (no host read)."""
    from . import augment as A
    columns, rows, jitter = columns or {}, rows or {}, jitter or {}
    for lk in list(dict.fromkeys(list(jitter) + list(columns) + list(rows))):
        i, k = lk
        a = _f32(nag[i][k], k)
        mask = columns.get(lk)
        row = rows.get(lk)
        if to_mean:
            if lk in jitter:
                A.jitter_(a, *jitter[lk][:2], seed=jitter[lk][2])
            out = a if inplace else a.clone()
            mean = a.mean(dim=0)
            if mask is not None:
                sel = torch.tensor([(mask >> j) & 1 == 1 for j in range(mean.numel())],
                                   device=a.device)
                out = torch.where(sel.view(1, -1) if a.dim() == 2 else sel, mean, out)
            if row is not None:
                n = a.shape[0]
                sel = A.unit(row[1], torch.arange(n, device=a.device)) < \
                    torch.tensor(row[0], dtype=torch.float32, device=a.device)
                out = torch.where(sel.view(-1, *([1] * (a.dim() - 1))), mean, out)
            if inplace:
                a.copy_(out)
            else:
                nag[i][k] = out
            continue
        out = None if inplace else torch.empty_like(a)
        A.features_(a, jitter=jitter.get(lk), col_mask=mask,
                    p_rows=None if row is None else row[0],
                    seed_rows=None if row is None else row[1], out=out)
        if out is not None:
            nag[i][k] = out
    return nag


class NAGDropoutColumns:
    """``NAGDropoutColumns`` (src/transforms/data.py:440-543, src/utils/dropout.py:7-22): every
    column of ``nag[i][key]`` is zeroed (set to its mean with ``to_mean``) with probability
    ``p``.  ``p <= 0`` does nothing.  At a level, the first MISSING key ends that level - the
    early ``return`` of ``DropoutColumns._process`` (data.py:470-472).  ``inplace=False`` writes a
    new tensor.

    ``draw``: ``torch.rand(n_cols) < p`` per (level, key), levels in order, keys in order."""

    def __init__(self, level="all", p=0.5, key=None, inplace=False, to_mean=False):
        assert isinstance(level, int) or level == "all" or level.endswith("-") \
            or level.endswith("+")
        self.level, self.p = level, p
        self.key = [key] if isinstance(key, str) else key
        self.inplace, self.to_mean = inplace, to_mean

    def draw(self, nag):
        params = {}
        if self.p <= 0:
            return params
        on = _per_level(self.level, False, True, nag.num_levels)
        for i in range(nag.num_levels):
            if not on[i]:
                continue
            for k in self.key:
                a = nag[i].get(k)
                if a is None:
                    break
                if a.dim() != 2:
                    raise IndexError(f"column dropout needs an [n, c] tensor, '{k}' is {tuple(a.shape)}")
                c = a.shape[1]
                if c > 64:
                    raise ValueError("column dropout handles at most 64 columns")
                drop = (torch.rand(c) < self.p).tolist()
                params[(i, k)] = sum(1 << j for j, f in enumerate(drop) if f)
        return params

    def apply(self, nag, params):
        return _dropout_apply(nag, columns=params, inplace=self.inplace, to_mean=self.to_mean)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class NAGDropoutRows:
    """``NAGDropoutRows`` (src/transforms/data.py:546-648): every row of ``nag[i][key]`` is zeroed
    (set to the column means with ``to_mean``) with probability ``p``; ``p <= 0`` does nothing;
    ``inplace=False`` writes a new tensor.

    One deliberate difference: with several keys and ``p > 0`` the reference builds one transform
    per (level, key) and trips the length assertion of ``NAG.apply_data_transform``
    (data.py:633-646, nag.py:816).  Here every present (level, key) pair gets its own draw.

    ``draw``: one ``segment._draw_seed()`` per present (level, key); row ``r`` is dropped when
    ``u(seed, r) < p``."""

    def __init__(self, level="all", p=0.5, key=None, inplace=False, to_mean=False):
        assert isinstance(level, int) or level == "all" or level.endswith("-") \
            or level.endswith("+")
        self.level, self.p = level, p
        self.key = [key] if isinstance(key, str) else key
        self.inplace, self.to_mean = inplace, to_mean

    def draw(self, nag):
        from .segment import _draw_seed
        params = {}
        if self.p <= 0:
            return params
        on = _per_level(self.level, False, True, nag.num_levels)
        for i in range(nag.num_levels):
            for k in self.key:
                if on[i] and nag[i].get(k) is not None:
                    params[(i, k)] = (float(self.p), _draw_seed())
        return params

    def apply(self, nag, params):
        return _dropout_apply(nag, rows=params, inplace=self.inplace, to_mean=self.to_mean)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


def _color_targets(data, keys, x_idx):
    """[(name, tensor view)] a ColorTransform touches (src/transforms/point.py:387-400)."""
    out = []
    if x_idx is None:
        for key in keys:
            for k in (key, f"mean_{key}"):
                t = data.get(k)
                if t is not None:
                    out.append((k, t))
    elif data.x is not None:
        out.append((("x", x_idx), data.x[:, x_idx:x_idx + 3]))
    return out


def _color_view(data, name):
    return data.x[:, name[1]:name[1] + 3] if isinstance(name, tuple) else data[name]


def _color_apply(nag, jitter=None, contrast=None, drop=None, new_tensor=False):
    """``jitter`` {(level, name): (sigma, trunc, seed)}, ``contrast`` {(level, name): (blend,
    1 - blend)}, ``drop`` {(level, name)}: one launch per tensor touched, plus the range launch of
    a tensor that is contrasted."""
    from . import augment as A
    jitter, contrast, drop = jitter or {}, contrast or {}, drop or {}
    for ln in list(dict.fromkeys(list(jitter) + list(contrast) + list(drop))):
        i, name = ln
        c = _f32(_color_view(nag[i], name), str(name))
        out = torch.empty_like(c) if new_tensor and not isinstance(name, tuple) else None
        A.color_(c, jitter=jitter.get(ln), contrast=contrast.get(ln), drop=ln in drop, out=out)
        if out is not None:
            nag[i][name] = out
    return nag


class NAGColorAutoContrast:
    """``NAGColorAutoContrast`` (src/transforms/point.py:409-488): with probability ``p``,
    ``rgb <- (1 - blend) * rgb + blend * (rgb - lo) / (hi - lo)`` with the per-column range of the
    tensor.  Acts on ``rgb`` and ``mean_rgb`` (``KEYS = ['rgb']``), or on ``x[:, x_idx:x_idx + 3]``
    in place.  Every tensor draws its OWN decision and, when ``blend is None``, its own blend
    (``_func`` runs once per tensor).  A constant column gives the reference's NaN (0 / 0).

    ``draw``: levels in order, tensors in the reference's order (key, then ``mean_`` key): one
    ``torch.rand(1)`` per tensor (also at levels ``level`` excludes, where p = -1 never takes
    it), then one more ``torch.rand(1)`` for the blend when it is taken and ``blend is None``."""
    KEYS = ["rgb"]

    def __init__(self, p=0.2, blend=None, x_idx=None, level="all"):
        self.p, self.blend, self.x_idx, self.level = p, blend, x_idx, level

    def draw(self, nag):
        level_p = _per_level(self.level, -1, self.p, nag.num_levels)
        params = {}
        for i in range(nag.num_levels):
            for name, _ in _color_targets(nag[i], self.KEYS, self.x_idx):
                if not bool(torch.rand(1) < level_p[i]):
                    continue
                if self.blend is None:
                    b = torch.rand(1)
                    params[(i, name)] = (float(b), float(1 - b))
                else:
                    params[(i, name)] = (float(self.blend), 1.0 - float(self.blend))
        return params

    def apply(self, nag, params):
        return _color_apply(nag, contrast=params, new_tensor=True)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class NAGColorDrop:
    """``NAGColorDrop`` (src/transforms/point.py:491-545): with probability ``p`` a colour tensor
    is multiplied by 0 in place (``rgb *= 0``: negative values give -0, NaN stays NaN).  Acts on
    ``rgb``, ``lab``, ``hsv`` and their ``mean_`` twins, or on ``x[:, x_idx:x_idx + 3]``; every
    tensor draws its own decision.

    ``draw``: one ``torch.rand(1)`` per tensor, levels in order, keys ``rgb, mean_rgb, lab,
    mean_lab, hsv, mean_hsv``."""
    KEYS = ["rgb", "lab", "hsv"]

    def __init__(self, p=0.2, x_idx=None, level="all"):
        self.p, self.x_idx, self.level = p, x_idx, level

    def draw(self, nag):
        level_p = _per_level(self.level, -1, self.p, nag.num_levels)
        params = {}
        for i in range(nag.num_levels):
            for name, _ in _color_targets(nag[i], self.KEYS, self.x_idx):
                if bool(torch.rand(1) < level_p[i]):
                    params[(i, name)] = True
        return params

    def apply(self, nag, params):
        return _color_apply(nag, drop=params)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class GeometricAugmentation:
    """``NAGJitterKey('pos', pos_jitter, trunc)`` + ``RandomTiltAndRotate(phi, theta)`` +
    ``RandomAnisotropicScale(delta)`` + ``RandomAxisFlip(flip_axis, flip_p)`` (default.yaml:
    250-264) as one launch per tensor.  ``draw`` is the four ``draw``s in that order, so under one
    ``torch.manual_seed`` the result equals the stepwise chain bit for bit."""

    def __init__(self, pos_jitter=0.01, trunc=0.05, phi=5, theta=180, delta=0.2, flip_axis=0,
                 flip_p=0.5):
        self.jitter = NAGJitterKey(key="pos", sigma=pos_jitter, trunc=trunc)
        self.tilt = RandomTiltAndRotate(phi=phi, theta=theta)
        self.scale = RandomAnisotropicScale(delta=delta)
        self.flip = RandomAxisFlip(axis=flip_axis, p=flip_p)

    def draw(self, nag):
        return {"jitter": self.jitter.draw(nag), "tilt": self.tilt.draw(nag),
                "scale": self.scale.draw(nag), "flip": self.flip.draw(nag)}

    def apply(self, nag, params):
        jitter = {i: v for (i, _), v in params["jitter"].items()}
        return _geometry_apply(nag, jitter=jitter, tilt=params["tilt"], scale=params["scale"],
                               flip=params["flip"])

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class FeatureAugmentation:
    """``NAGJitterKey(key, sigma, trunc)`` + ``NAGDropoutColumns(p=p_columns, key=key,
    inplace=True)`` + ``NAGDropoutRows(p=p_rows, key=key, inplace=True)`` (default.yaml:293-340
    for one group of keys) as one launch per tensor, in place.  ``draw`` is the three ``draw``s in
    that order."""

    def __init__(self, key=None, sigma=0.01, trunc=0.02, p_columns=0.0, p_rows=0.0, level="all"):
        self.jitter = NAGJitterKey(key=key, sigma=sigma, trunc=trunc)
        self.columns = NAGDropoutColumns(level=level, p=p_columns, key=key, inplace=True)
        self.rows = NAGDropoutRows(level=level, p=p_rows, key=key, inplace=True)

    def draw(self, nag):
        return {"jitter": self.jitter.draw(nag), "columns": self.columns.draw(nag),
                "rows": self.rows.draw(nag)}

    def apply(self, nag, params):
        return _dropout_apply(nag, columns=params["columns"], rows=params["rows"],
                              jitter=params["jitter"], inplace=True)

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class ColorAugmentation:
    """``NAGJitterKey('rgb', sigma, trunc)`` + ``NAGColorAutoContrast(p_contrast, blend)`` +
    ``NAGColorDrop(p_drop)`` (default.yaml:348-358) as one launch per tensor touched, plus the
    range launch of a tensor that is contrasted (the range is that of the JITTERED colours, which
    the range kernel recomputes instead of storing).  ``draw`` is the three ``draw``s in that
    order."""

    def __init__(self, sigma=0.01, trunc=0.02, p_contrast=0.2, blend=None, p_drop=0.2,
                 level="all"):
        self.jitter = NAGJitterKey(key="rgb", sigma=sigma, trunc=trunc)
        self.contrast = NAGColorAutoContrast(p=p_contrast, blend=blend, level=level)
        self.drop = NAGColorDrop(p=p_drop, level=level)

    def draw(self, nag):
        return {"jitter": self.jitter.draw(nag), "contrast": self.contrast.draw(nag),
                "drop": self.drop.draw(nag)}

    def apply(self, nag, params):
        return _color_apply(nag, jitter=params["jitter"], contrast=params["contrast"],
                            drop=params["drop"])

    def __call__(self, nag):
        return self.apply(nag, self.draw(nag))


class QuantizePointCoordinates:
    """``QuantizePointCoordinates`` (src/transforms/sampling.py:507-568): the integer voxel
    coordinates the sparse CNN runs on, computed on the fly because the augmentations move the
    points.  ``size <= 0``: nothing happens.  Otherwise one point per voxel of ``size`` is kept -
    ``voxel.voxel_groups(pos, size, batch).last``, the highest point index of each voxel in
    ascending voxel order (PyG's ``consecutive_cluster`` on the CPU) - through
    ``nag.select(0, ...)``, and level 0 gets ``coords`` = ``round(pos / size)`` of the kept points
    as floats, shifted to a zero minimum per axis unless ``allow_negative_coords``."""

    def __init__(self, size, allow_negative_coords=False):
        self.grid_size = size
        self.allow_negative_coords = allow_negative_coords

    def __call__(self, nag):
        if self.grid_size <= 0:
            return nag
        from .voxel import voxel_groups
        data = nag[0]
        pos = data.pos
        kept = voxel_groups(pos, self.grid_size, data.get("batch")).last
        coords = torch.round(pos / self.grid_size)[kept]
        out = nag.select(0, kept)
        if not self.allow_negative_coords:
            coords = coords - coords.min(dim=0, keepdim=True).values
        out[0].coords = coords
        return out


class PretrainedCNN:
    """``PretrainedCNN`` (src/transforms/point.py:630-770): runs a trained first stage (a
    ``PointStage`` with ``cnn_blocks=True``) over a level-0 ``Data`` at preprocessing time and
    leaves its output in ``data.x``, the features the partition reads.  ``load_checkpoint`` takes
    the keys of ``checkpoint['state_dict']`` that contain ``first_stage``, strips
    ``net.first_stage.`` and raises ``ValueError`` on a shape mismatch; keys the module lacks are
    left out, parameters the checkpoint lacks keep their values."""

    def __init__(self, first_stage, ckpt_path, partition_hf=None, norm_mode="graph", device="cuda",
                 verbose=False):
        assert partition_hf is not None, "`partition_hf` has not been set up."
        self.norm_mode, self.ckpt_path, self.partition_hf = norm_mode, ckpt_path, partition_hf
        self.device, self.verbose = device, verbose
        first_stage.to(device)
        self.first_stage = self.load_checkpoint(first_stage, ckpt_path, device, verbose=verbose)

    def __call__(self, data):
        from .nn.spt import SPT
        with torch.no_grad():
            # the partition_hf keys stay: they are saved to disk for training
            data.add_keys_to(keys=self.partition_hf, to="x", delete_after=False)
            x, _ = SPT.forward_first_stage(data=data, first_stage=self.first_stage,
                                           use_node_hf=True, norm_mode=self.norm_mode)
            data.x = x
        return data

    _process = __call__

    @staticmethod
    def load_checkpoint(first_stage, ckpt_path, device, verbose=False):
        import os
        assert ckpt_path is not None and os.path.exists(ckpt_path), \
            f"Expected a valid checkpoint path. Received {ckpt_path=}"
        checkpoint = torch.load(ckpt_path, map_location=device)
        model_dict = first_stage.state_dict()
        ckpt_dict = {k.replace("net.first_stage.", ""): v
                     for k, v in checkpoint["state_dict"].items() if "first_stage" in k}
        loadable, unused = {}, {}
        for k, v in ckpt_dict.items():
            if k not in model_dict:
                unused[k] = v
            elif v.shape != model_dict[k].shape:
                raise ValueError(f"Shape mismatch for {k}: checkpoint {v.shape} vs model "
                                 f"{model_dict[k].shape}")
            else:
                loadable[k] = v
        missing = [k for k in model_dict if k not in loadable]
        model_dict.update(loadable)
        first_stage.load_state_dict(model_dict)
        if verbose:
            print(f"PretrainedCNN: loaded {len(loadable)} parameters ({', '.join(loadable)}); "
                  f"{len(unused)} unused in the checkpoint ({', '.join(unused)}); {len(missing)} "
                  f"missing from it ({', '.join(missing)})")
        return first_stage
