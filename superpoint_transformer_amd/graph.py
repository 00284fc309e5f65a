"""Superedge construction helpers of the preprocessing graph stage
(src/utils/graph.py, src/utils/edge.py, src/utils/sparse.py) on the HIP ops.

``subedges`` (graph.py:99-463) finds, for every edge between two segments, the level-0 point
pairs that "make up" the edge - the input of the superedge features.  The reference strings
~25 torch / torch_scatter calls over edge-wise expanded point lists; the same steps run here
with every segment-wise reduction on the CSR kernels (segment sum / min / max / mean,
``scatter_pca``) and the anchor search on ``spt_cluster_pair_anchors_f32``; the expansions,
masks and the per-group sorts are index plumbing (torch sorts on composite keys).
"""
import torch

from . import _lib
from .csr import csr_of
from .ops import segment_reduce

__all__ = ["to_trimmed", "edge_wise_points", "base_vectors_3d", "subedges",
           "partition_adjacency", "PartitionGraph", "superedge_features", "superedge_capacity",
           "minimalistic_edge_features", "connect_isolated"]


def to_trimmed(edge_index):
    """Undirected, duplicate-free, loop-free edges with i < j, sorted by (i, j)
    (graph.py:466-502: flip, coalesce, remove_self_loops)."""
    lo = torch.minimum(edge_index[0], edge_index[1])
    hi = torch.maximum(edge_index[0], edge_index[1])
    keep = lo != hi
    lo, hi = lo[keep], hi[keep]
    n = int(hi.max()) + 1 if hi.numel() else 1
    key = torch.unique(lo * n + hi, sorted=True)
    return torch.stack([key // n, key % n])


def base_vectors_3d(x):
    """Orthonormal bases whose first vector is ``x`` normalised (geometry.py:42-78); the two
    degenerate cases get the reference's arbitrary fill-ins."""
    a = x.clone()
    zero = a.norm(dim=1) == 0
    a[zero] = torch.tensor([1.0, 0.0, 0.0], dtype=x.dtype, device=x.device)
    a = a / a.norm(dim=1).view(-1, 1)
    b = torch.stack((a[:, 1] - a[:, 2], a[:, 2] - a[:, 0], a[:, 0] - a[:, 1]), dim=1)
    zb = b.norm(dim=1) == 0
    b[zb] = torch.tensor([2.0, 1.0, -1.0], dtype=x.dtype, device=x.device)
    b = b / b.norm(dim=1).view(-1, 1)
    c = torch.linalg.cross(a, b)
    return torch.stack((a, b, c), dim=1)


def _arange_interleave(width, start):
    """cat([arange(s, s + w) for s, w in zip(start, width)]) (tensor.py:122-140)."""
    total = int(width.sum())
    if total == 0:
        return torch.empty(0, dtype=torch.long, device=width.device)
    grp = torch.repeat_interleave(torch.arange(width.numel(), device=width.device), width)
    first = torch.cumsum(width, 0) - width
    return start[grp] + torch.arange(total, device=width.device) - first[grp]


def edge_wise_points(points, index, edge_index, num_segments=None):
    """For every edge, all points of its source segment and all points of its target segment
    (edge.py:22-77): ``((S_points, S_idx, S_uid), (T_points, T_idx, T_uid))``; edges are
    identified by their rank in (source, target) order."""
    if index.is_cuda:
        csr = csr_of(index, num_segments)
        pointers, order = csr.rowptr.long(), csr.perm.long()
    else:                                               # the same view, by a stable sort
        num = int(index.max()) + 1 if num_segments is None else int(num_segments)
        order = torch.argsort(index, stable=True)
        pointers = torch.zeros(num + 1, dtype=torch.long)
        pointers[1:] = torch.cumsum(torch.bincount(index, minlength=num), 0)
    size = pointers[1:] - pointers[:-1]
    n = max(int(edge_index.max()) + 1 if edge_index.numel() else 1, 1)
    uid = torch.unique(edge_index[0] * n + edge_index[1], sorted=True, return_inverse=True)[1]

    def expand(x_idx):
        sz = size[x_idx]
        pid = order[_arange_interleave(sz, pointers[:-1][x_idx])]
        return points[pid], pid, torch.repeat_interleave(uid, sz)

    return expand(edge_index[0]), expand(edge_index[1])


def _group_sort(value, group, descending=False):
    """Order by group first, ``value`` second (sparse.py:90-104: ``sparse_sort``): two stable
    sorts on exact keys instead of one sort on a normalised float key."""
    p1 = torch.argsort(value, descending=descending, stable=True)
    p2 = torch.argsort(group[p1], stable=True)
    return p1[p2]


def _preserving(mask, uid, num):
    """``idx_preserving_mask`` (scatter.py:241-246): never empty a group entirely."""
    kept = segment_reduce(mask.float().view(-1, 1), uid, num, "sum").view(-1)
    return mask | (kept == 0)[uid]


def subedges(points, index, edge_index, ratio=0.2, k_min=20, cycles=3, pca_on_cpu=False,
             margin=0.2, halfspace_filter=True, bbox_filter=True, target_pc_flip=True,
             source_pc_sort=False, chunk_size=None, verbose=False):
    """graph.py:99-463.  Returns ``(edge_index [2,E] trimmed, ST_pairs [2,M], ST_uid [M])``:
    pair m joins point ``ST_pairs[0,m]`` of the source segment with ``ST_pairs[1,m]`` of the
    target segment of edge ``ST_uid[m]``.  ``chunk_size`` / ``pca_on_cpu`` are accepted and
    ignored (nothing here needs chunking, the PCA is a kernel).  CPU tensors take the same steps on
    torch alone (``_subedges_torch``)."""
    from .neighbors import _pair_anchors
    from .segment import scatter_pca
    if not points.is_cuda:
        return _subedges_torch(points, index, edge_index, ratio, k_min, cycles, margin,
                               halfspace_filter, bbox_filter, target_pc_flip, source_pc_sort)
    _lib.require_cuda(points, index, edge_index)
    points = points.detach().float().contiguous()
    index = index.long().contiguous()
    edge_index = to_trimmed(edge_index.long())
    E = edge_index.shape[1]
    dev = points.device
    if E == 0:
        z = torch.empty(0, dtype=torch.long, device=dev)
        return edge_index, torch.stack([z, z]), z
    num_segments = int(index.max()) + 1

    # closest pair of points of the two segments: origin and first axis of the edge's frame
    anchors, _ = _pair_anchors(points, index, edge_index, cycles, num_segments)
    s_anchor, t_anchor = points[anchors[0]], points[anchors[1]]
    base = base_vectors_3d(t_anchor - s_anchor)                      # [E,3,3], rows = axes

    (S_pts, S_idx, S_uid), (T_pts, T_idx, T_uid) = edge_wise_points(points, index, edge_index,
                                                                   num_segments)

    def to_anchor_base(X, uid, anchor):
        return torch.einsum("nd,nkd->nk", X - anchor[uid], base[uid])

    S_pts = to_anchor_base(S_pts, S_uid, s_anchor)
    T_pts = to_anchor_base(T_pts, T_uid, t_anchor)

    def take(mask, P, I, U):
        keep = torch.where(_preserving(mask, U, E))[0]
        return P[keep], I[keep], U[keep]

    if halfspace_filter:                                             # graph.py:297-312
        S_pts, S_idx, S_uid = take(S_pts[:, 0] <= margin, S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(T_pts[:, 0] >= -margin, T_pts, T_idx, T_uid)

    if bbox_filter:                                                  # graph.py:325-350
        s_min = segment_reduce(S_pts[:, 1:].contiguous(), S_uid, E, "min")
        s_max = segment_reduce(S_pts[:, 1:].contiguous(), S_uid, E, "max")
        t_min = segment_reduce(T_pts[:, 1:].contiguous(), T_uid, E, "min")
        t_max = segment_reduce(T_pts[:, 1:].contiguous(), T_uid, E, "max")
        st_min = torch.max(s_min, t_min).clamp(max=-margin)
        st_max = torch.min(s_max, t_max).clamp(min=margin)

        def in_bbox(P, U):
            return (P[:, 1:] >= st_min[U]).all(dim=1) & (P[:, 1:] <= st_max[U]).all(dim=1)
        S_pts, S_idx, S_uid = take(in_bbox(S_pts, S_uid), S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(in_bbox(T_pts, T_uid), T_pts, T_idx, T_uid)

    # closest to the anchor first, along the edge direction (graph.py:359-370)
    p = _group_sort(S_pts[:, 0], S_uid, descending=True)
    S_pts, S_idx, S_uid = S_pts[p], S_idx[p], S_uid[p]
    p = _group_sort(T_pts[:, 0], T_uid, descending=False)
    T_pts, T_idx, T_uid = T_pts[p], T_idx[p], T_uid[p]

    # top `ratio` of the points, at least k_min, the same number on both sides (graph.py:379-399)
    s_size = torch.bincount(S_uid, minlength=E)
    t_size = torch.bincount(T_uid, minlength=E)
    s_k = (s_size * ratio).long().clamp(min=k_min).min(s_size)
    t_k = (t_size * ratio).long().clamp(min=k_min).min(t_size)
    st_k = torch.min(s_k, t_k)
    sel = _arange_interleave(st_k, torch.cumsum(s_size, 0) - s_size)
    S_pts, S_idx, S_uid = S_pts[sel], S_idx[sel], S_uid[sel]
    sel = _arange_interleave(st_k, torch.cumsum(t_size, 0) - t_size)
    T_pts, T_idx, T_uid = T_pts[sel], T_idx[sel], T_uid[sel]

    # first principal component of each side's selected points (graph.py:415-428)
    s_v = scatter_pca(S_pts.contiguous(), S_uid, E)[1][:, :, -1].contiguous()
    t_v = scatter_pca(T_pts.contiguous(), T_uid, E)[1][:, :, -1].contiguous()

    if target_pc_flip and not source_pc_sort:                        # graph.py:437-444
        T_proj = (T_pts * t_v[T_uid]).sum(dim=1)
        s_mean = segment_reduce(S_pts.contiguous(), S_uid, E, "mean")
        _, amin = segment_reduce(T_proj.view(-1, 1).contiguous(), T_uid, E, "min", return_arg=True)
        t_minp = T_pts[amin.view(-1).long().clamp(max=max(T_pts.shape[0] - 1, 0))]
        st_u = t_minp - s_mean
        st_u = st_u / st_u.norm(dim=1).view(-1, 1)
        flip = (s_v * t_v).sum(dim=1) <= (s_v * st_u).sum(dim=1)
        t_v = torch.where(flip.view(-1, 1), -t_v, t_v)
    elif source_pc_sort:
        t_v = s_v

    def sort_along(P, I, U, v):                                      # sparse.py:107-137
        centroid = segment_reduce(P.contiguous(), U, E, "mean")
        proj = ((P - centroid[U]) * v[U]).sum(dim=1)
        q = _group_sort(proj, U, descending=False)
        return I[q], U[q]

    S_idx, S_uid = sort_along(S_pts, S_idx, S_uid, s_v)
    T_idx, T_uid = sort_along(T_pts, T_idx, T_uid, t_v)
    return edge_index, torch.vstack((S_idx, T_idx)), S_uid


# ---------------------------------------------------------------------------
# The same rules in plain torch: the route of CPU tensors
# ---------------------------------------------------------------------------
def _gsum(x, uid, num):
    out = torch.zeros((num,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    return out.index_add_(0, uid, x)


def _gext(x, uid, num, red):
    out = torch.zeros((num,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    index = uid.view([-1] + [1] * (x.dim() - 1)).expand_as(x)
    return out.scatter_reduce(0, index, x, red, include_self=False)


def _gargmin(value, uid, num):
    """Position of every group's first smallest value."""
    vmin = _gext(value, uid, num, "amin")
    where = torch.arange(value.numel(), device=value.device)
    where = torch.where(value == vmin[uid], where, torch.full_like(where, value.numel()))
    return _gext(where, uid, num, "amin")


def _pair_anchors_torch(points, index, edge_index, cycles, num_segments):
    """``scatter_nearest_neighbor`` (src/utils/scatter.py:128-238) as ``neighbors._pair_anchors``
    runs it: start at the centroids, ``cycles`` rounds of nearest-in-target, nearest-in-source;
    ties to the first point in ascending order."""
    E = edge_index.shape[1]
    cnt = torch.bincount(index, minlength=num_segments).clamp(min=1).view(-1, 1)
    centroid = (_gsum(points.double(), index, num_segments) / cnt).to(points.dtype)
    (S_pts, S_idx, S_uid), (T_pts, T_idx, T_uid) = edge_wise_points(points, index, edge_index,
                                                                   num_segments)
    sc = centroid[edge_index[0]]
    si = ti = None
    for _ in range(int(cycles)):
        ti = T_idx[_gargmin((T_pts - sc[T_uid]).norm(dim=1), T_uid, E)]
        tc = points[ti]
        si = S_idx[_gargmin((S_pts - tc[S_uid]).norm(dim=1), S_uid, E)]
        sc = points[si]
    return torch.stack((si, ti))


def _pca_first_component(P, uid, num):
    """Last column of ``scatter_pca``'s eigenvectors: f64 population covariance, ``eigh``."""
    x = P.double()
    cnt = torch.bincount(uid, minlength=num).clamp(min=1).view(-1, 1).double()
    mean = _gsum(x, uid, num) / cnt
    d = x - mean[uid]
    cov = _gsum(d.unsqueeze(2) * d.unsqueeze(1), uid, num) / cnt.view(-1, 1, 1)
    return torch.linalg.eigh(cov)[1][:, :, -1].to(P.dtype)


def _subedges_torch(points, index, edge_index, ratio=0.2, k_min=20, cycles=3, margin=0.2,
                    halfspace_filter=True, bbox_filter=True, target_pc_flip=True,
                    source_pc_sort=False, dtype=torch.float32):
    """``subedges`` step by step on torch alone (any device; the route of CPU tensors)."""
    points = points.detach().to(dtype).contiguous()
    index = index.long().contiguous()
    edge_index = to_trimmed(edge_index.long())
    E = edge_index.shape[1]
    if E == 0:
        z = torch.empty(0, dtype=torch.long, device=points.device)
        return edge_index, torch.stack([z, z]), z
    num_segments = int(index.max()) + 1
    anchors = _pair_anchors_torch(points, index, edge_index, cycles, num_segments)
    s_anchor, t_anchor = points[anchors[0]], points[anchors[1]]
    base = base_vectors_3d(t_anchor - s_anchor)
    (S_pts, S_idx, S_uid), (T_pts, T_idx, T_uid) = edge_wise_points(points, index, edge_index,
                                                                   num_segments)

    def to_anchor_base(X, uid, anchor):
        d, b = X - anchor[uid], base[uid]
        return torch.stack([(d[:, 0] * b[:, k, 0] + d[:, 1] * b[:, k, 1]) + d[:, 2] * b[:, k, 2]
                            for k in range(3)], dim=1)

    S_pts = to_anchor_base(S_pts, S_uid, s_anchor)
    T_pts = to_anchor_base(T_pts, T_uid, t_anchor)

    def take(mask, P, I, U):
        kept = _gsum(mask.long(), U, E)
        keep = torch.where(mask | (kept == 0)[U])[0]
        return P[keep], I[keep], U[keep]

    if halfspace_filter:
        S_pts, S_idx, S_uid = take(S_pts[:, 0] <= margin, S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(T_pts[:, 0] >= -margin, T_pts, T_idx, T_uid)
    if bbox_filter:
        st_min = torch.max(_gext(S_pts[:, 1:], S_uid, E, "amin"),
                           _gext(T_pts[:, 1:], T_uid, E, "amin")).clamp(max=-margin)
        st_max = torch.min(_gext(S_pts[:, 1:], S_uid, E, "amax"),
                           _gext(T_pts[:, 1:], T_uid, E, "amax")).clamp(min=margin)

        def in_bbox(P, U):
            return (P[:, 1:] >= st_min[U]).all(dim=1) & (P[:, 1:] <= st_max[U]).all(dim=1)
        S_pts, S_idx, S_uid = take(in_bbox(S_pts, S_uid), S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(in_bbox(T_pts, T_uid), T_pts, T_idx, T_uid)

    p = _group_sort(S_pts[:, 0], S_uid, descending=True)
    S_pts, S_idx, S_uid = S_pts[p], S_idx[p], S_uid[p]
    p = _group_sort(T_pts[:, 0], T_uid, descending=False)
    T_pts, T_idx, T_uid = T_pts[p], T_idx[p], T_uid[p]

    s_size = torch.bincount(S_uid, minlength=E)
    t_size = torch.bincount(T_uid, minlength=E)
    s_k = (s_size * ratio).long().clamp(min=k_min).min(s_size)
    t_k = (t_size * ratio).long().clamp(min=k_min).min(t_size)
    st_k = torch.min(s_k, t_k)
    sel = _arange_interleave(st_k, torch.cumsum(s_size, 0) - s_size)
    S_pts, S_idx, S_uid = S_pts[sel], S_idx[sel], S_uid[sel]
    sel = _arange_interleave(st_k, torch.cumsum(t_size, 0) - t_size)
    T_pts, T_idx, T_uid = T_pts[sel], T_idx[sel], T_uid[sel]

    s_v = _pca_first_component(S_pts, S_uid, E)
    t_v = _pca_first_component(T_pts, T_uid, E)
    kk = st_k.clamp(min=1).view(-1, 1)

    def mean_of(P, U):
        return (_gsum(P.double(), U, E) / kk).to(P.dtype)

    if target_pc_flip and not source_pc_sort:
        T_proj = (T_pts * t_v[T_uid]).sum(dim=1)
        t_minp = T_pts[_gargmin(T_proj, T_uid, E)]
        st_u = t_minp - mean_of(S_pts, S_uid)
        st_u = st_u / st_u.norm(dim=1).view(-1, 1)
        flip = (s_v * t_v).sum(dim=1) <= (s_v * st_u).sum(dim=1)
        t_v = torch.where(flip.view(-1, 1), -t_v, t_v)
    elif source_pc_sort:
        t_v = s_v

    def sort_along(P, I, U, v):
        proj = ((P - mean_of(P, U)[U]) * v[U]).sum(dim=1)
        q = _group_sort(proj, U, descending=False)
        return I[q], U[q]

    S_idx, S_uid = sort_along(S_pts, S_idx, S_uid, s_v)
    T_idx, T_uid = sort_along(T_pts, T_idx, T_uid, t_v)
    return edge_index, torch.vstack((S_idx, T_idx)), S_uid


# ---------------------------------------------------------------------------
# Superedges: subedges and the stored edge features in one kernel
# ---------------------------------------------------------------------------
def minimalistic_edge_features(pos, pairs, uid, num_edges):
    """The 7 stored features of every edge from its point pairs
    (``_minimalistic_horizontal_edge_features``, src/transforms/graph.py:950-1060):
    ``mean_off`` [3], ``std_off`` [3] (unbiased ``scatter_std`` of the offsets in
    ``base_vectors_3d(mean_off)``, clipped to [-2, 2]; one pair gives 0), ``mean_dist`` =
    sqrt(mean(norm(offset))), in ``pos``'s dtype.  ``uid`` [M] names the edge of every pair.  On
    the device the f32 group sums are the CSR kernels', so two runs are bit-equal."""
    E = int(num_edges)
    pairs, uid = pairs.long(), uid.long()
    if pos.is_cuda and pos.dtype == torch.float32 and uid.numel():
        def gsum(x):
            return segment_reduce(x.contiguous(), uid, E, "sum")
    else:
        def gsum(x):
            return _gsum(x, uid, E)
    offset = pos[pairs[1]] - pos[pairs[0]]
    cnt = torch.bincount(uid, minlength=E).clamp(min=1).to(pos.dtype).view(-1, 1)
    mean_off = gsum(offset) / cnt
    base = base_vectors_3d(mean_off)[uid]
    uvw = torch.stack([(offset * base[:, k]).sum(dim=1) for k in range(3)], dim=1)
    dev = uvw - (gsum(uvw) / cnt)[uid]
    std_off = (gsum(dev * dev) / ((cnt - 1).clamp(min=1) + 1e-6)).sqrt().clip(-2, 2)
    mean_dist = (gsum(offset.norm(dim=1).view(-1, 1)) / cnt).sqrt()
    return torch.cat((mean_off, std_off, mean_dist), dim=1)


def connect_isolated(edge_index, pos, k, batch=None, num_nodes=None):
    """``Data.connect_isolated(k)`` for a graph without ``edge_attr`` (src/data/data.py:481-524):
    every node no edge touches gets edges to its ``k`` nearest other nodes (within its cloud
    when ``batch`` is given), appended to ``edge_index``."""
    N = pos.shape[0] if num_nodes is None else int(num_nodes)
    linked = torch.zeros(N, dtype=torch.bool, device=pos.device)
    linked[edge_index.flatten()] = True
    is_out = torch.where(~linked)[0]
    if is_out.numel() == 0:
        return edge_index
    nb, _ = _isolated_edges(pos.detach().float().contiguous(), is_out, int(k), batch)
    source, target = is_out.repeat_interleave(int(k)), nb.flatten()
    found = target >= 0
    return torch.cat((edge_index, torch.stack((source[found], target[found]))), dim=1)


def superedge_capacity():
    """Most points a side of an edge may have for the workgroup kernel (``C`` of DESIGN 7.21)."""
    return int(_lib.lib.spt_superedge_capacity())


def superedge_features(pos, index, edge_index, ratio=0.2, k_min=20, cycles=3, margin=0.2,
                       halfspace_filter=True, bbox_filter=True, target_pc_flip=True,
                       source_pc_sort=False, return_pairs=False, num_segments=None):
    """``subedges`` and ``_minimalistic_horizontal_edge_features`` in one pass per edge
    (``csrc/superedge.hip``): returns ``(edge_index [2, E] trimmed, edge_attr [E, 7])`` and, with
    ``return_pairs``, ``(pairs [2, M], uid [M])`` as ``subedges`` gives them.

    ``pos`` [N0, 3] level-0 points, ``index`` [N0] their segment, ``edge_index`` [2, *] edges
    between segments (trimmed here).  Edges whose two segments hold at most 64 points take a wave
    each, up to ``superedge_capacity()`` points a workgroup with both sides in LDS; an edge with a
    larger side goes through ``subedges`` + ``minimalistic_edge_features`` and is merged back by
    edge id.  Host reads: the three class counts, and the number of pairs when they are asked
    for.  CPU tensors take the torch composition of the same rules."""
    if not pos.is_cuda:
        ei, pairs, uid = _subedges_torch(pos, index, edge_index, ratio, k_min, cycles, margin,
                                         halfspace_filter, bbox_filter, target_pc_flip,
                                         source_pc_sort)
        attr = minimalistic_edge_features(pos.detach().float(), pairs, uid, ei.shape[1])
        return (ei, attr, pairs, uid) if return_pairs else (ei, attr)
    from .neighbors import _pair_anchors
    from .ops import _workspace
    _lib.require_cuda(pos, index, edge_index)
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("pos must be [N, 3]")
    if pos.shape[0] > 2 ** 31 - 1:
        raise ValueError("superedge_features indexes points with 32 bits: more than 2^31 - 1 points")
    p = _lib.dense(pos.detach(), torch.float32)
    index = _lib.dense(index, torch.int64, 8)
    edge_index = to_trimmed(edge_index.long()).contiguous()
    E = edge_index.shape[1]
    dev = p.device
    if E == 0:
        z = torch.empty(0, dtype=torch.long, device=dev)
        attr = torch.empty((0, 7), dtype=torch.float32, device=dev)
        return (edge_index, attr, torch.stack([z, z]), z) if return_pairs else (edge_index, attr)
    if num_segments is None:
        num_segments = int(index.max()) + 1
    kw = dict(ratio=ratio, k_min=k_min, cycles=cycles, margin=margin,
              halfspace_filter=halfspace_filter, bbox_filter=bbox_filter,
              target_pc_flip=target_pc_flip, source_pc_sort=source_pc_sort)
    csr = csr_of(index, num_segments)
    anchors, _ = _pair_anchors(p, index, edge_index, cycles, num_segments)
    L = _lib.lib
    stream = _lib.stream_ptr(dev)
    nbytes = L.spt_superedge_workspace_bytes(E)

    order = torch.empty(E, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_superedge_classify(_lib.ptr(csr.rowptr), csr.num_seg, _lib.ptr(edge_index), E, E,
                                      _lib.ptr(order), _lib.ptr(counts), _lib.ptr(ws), nbytes, stream)
    _lib.check(st, "spt_superedge_classify")
    n_small, n_medium, n_large = counts.tolist()                  # host sync: the class counts

    edge_attr = torch.empty((E, 7), dtype=torch.float32, device=dev)
    count = torch.empty(E, dtype=torch.int32, device=dev)
    large = l_pairs = l_uid = l_count = None
    if n_large:                                                   # a side above the capacity
        large = order[n_small + n_medium:].long()
        sub = edge_index[:, large]
        if int(sub.max()) >= csr.num_seg or int(sub.min()) < 0:
            raise ValueError(f"edge_index names segments outside [0, {csr.num_seg})")
        _, l_pairs, l_uid = subedges(p, index, sub, **kw)
        l_count = torch.bincount(l_uid, minlength=n_large)
        edge_attr[large] = minimalistic_edge_features(p, l_pairs, l_uid, n_large)
        count[large] = l_count.int()

    switches = (1 if halfspace_filter else 0) | (2 if bbox_filter else 0) \
        | (4 if target_pc_flip else 0) | (8 if source_pc_sort else 0)

    def launch(count_only, offsets, pairs, uid, M):
        with torch.cuda.device(dev):
            st = L.spt_superedge_f32(_lib.ptr(p), p.shape[0], _lib.ptr(csr.perm), _lib.ptr(csr.rowptr),
                                     csr.num_seg, _lib.ptr(edge_index), E, E, _lib.ptr(anchors),
                                     _lib.ptr(order), n_small, n_medium, float(ratio), int(k_min),
                                     float(margin), switches, int(count_only), _lib.ptr(edge_attr),
                                     _lib.ptr(count), _lib.ptr(offsets), _lib.ptr(pairs),
                                     _lib.ptr(uid), M, stream)
        _lib.check(st, "spt_superedge_f32")

    if not return_pairs:
        launch(0, None, None, None, 0)
        return edge_index, edge_attr
    # the offsets must exist before a pair is written: a count-only launch (projection and filters
    # alone), the device scan, then the full launch
    launch(1, None, None, None, 0)
    M = int(count.sum())                                          # host sync: the number of pairs
    if M >= 2 ** 32:
        raise ValueError("more than 2^32 - 1 subedge pairs: split the edge list")
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)   # uint32 words
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_superedge_pair_offsets(_lib.ptr(count), E, _lib.ptr(offsets), _lib.ptr(ws), nbytes,
                                          stream)
    _lib.check(st, "spt_superedge_pair_offsets")
    pairs = torch.empty((2, M), dtype=torch.int64, device=dev)
    uid = torch.empty(M, dtype=torch.int64, device=dev)
    launch(0, offsets, pairs, uid, M)
    if n_large and l_uid.numel():
        first = (torch.cumsum(l_count, 0) - l_count)[l_uid]
        at = (offsets[:E][large].long() & 0xFFFFFFFF)[l_uid] \
            + torch.arange(l_uid.numel(), device=dev) - first
        pairs[:, at] = l_pairs
        uid[at] = large[l_uid]
    return edge_index, edge_attr, pairs, uid


# ---------------------------------------------------------------------------
# Input graph of the partition: kNN table -> trimmed, weighted forward star
# ---------------------------------------------------------------------------
_REDUCE_CODES = {"mean": 0, "add": 1, "sum": 1, "min": 2, "max": 3}


class PartitionGraph:
    """What ``partition_adjacency`` returns: ``edge_index`` [2, E] int64 (i < j, sorted by
    (i, j)), ``edge_attr`` [E] f32 or None, ``source_csr`` [N + 1] int64 (row pointers over
    ``edge_index[0]``) and ``num_isolated``.  ``target`` is ``edge_index[1]``; the forward
    star's ``reindex`` is the identity since the edges are sorted."""
    __slots__ = ("edge_index", "edge_attr", "source_csr", "num_isolated")

    def __init__(self, edge_index, edge_attr, source_csr, num_isolated):
        self.edge_index, self.edge_attr = edge_index, edge_attr
        self.source_csr, self.num_isolated = source_csr, int(num_isolated)

    @property
    def target(self):
        return self.edge_index[1]


def _regression_line(n, sd, sdd, sw, sdw):
    """Least-squares ``(a, b)`` of ``a d + b = w`` from the five sums (data.py:535-545).  A
    rank-deficient system (every distance equal) gets lstsq's minimum-norm solution."""
    det = n * sdd - sd * sd
    if n > 0 and det > 1e-12 * max(n * sdd, 1e-300):
        a = (n * sdw - sd * sw) / det
        return a, (sw - a * sd) / n
    if n <= 0:
        return 0.0, 0.0
    d0, w0 = sd / n, sw / n                      # rows all equal [d0, 1]: x = w0 [d0, 1] / (d0^2 + 1)
    return w0 * d0 / (d0 * d0 + 1.0), w0 / (d0 * d0 + 1.0)


def _knn_isolated_torch(pos, query, k, r_max, batch_search, batch_query):
    """``knn_2`` by exhaustive search, for CPU tensors: the k nearest within ``r_max`` (squared
    distance < r_max^2 in f32, ties by index, -1 padding; squared distances returned)."""
    s, q = pos.float(), query.float()
    if batch_search is not None:
        z = torch.cat((s[:, 2], q[:, 2]))
        zoff = z.max() - z.min() + r_max + 1
        s, q = s.clone(), q.clone()
        s[:, 2] += batch_search.to(s.dtype) * zoff
        q[:, 2] += batch_query.to(q.dtype) * zoff
    diff = q[:, None, :] - s[None, :, :]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    r2 = torch.tensor(float(r_max), dtype=torch.float32) ** 2
    d2 = torch.where(d2 < r2, d2, torch.full_like(d2, float("inf")))
    kk = min(k, s.shape[0])
    dsel, order = torch.sort(d2, dim=1, stable=True)
    dsel, order = dsel[:, :kk], order[:, :kk]
    nb = torch.full((q.shape[0], k), -1, dtype=torch.long, device=pos.device)
    dd = torch.full((q.shape[0], k), -1.0, dtype=torch.float32, device=pos.device)
    good = torch.isfinite(dsel)
    nb[:, :kk] = torch.where(good, order, torch.full_like(order, -1))
    dd[:, :kk] = torch.where(good, dsel, torch.full_like(dsel, -1.0))
    return nb, dd


def _coalesce_torch(edge_index, edge_attr, reduce):
    """``coalesce`` in plain torch, for CPU tensors (the device route uses the shims')."""
    n = int(edge_index.max()) + 1 if edge_index.numel() else 1
    uniq, inv = torch.unique(edge_index[0] * n + edge_index[1], sorted=True, return_inverse=True)
    ei = torch.stack([uniq // n, uniq % n])
    if edge_attr is None:
        return ei, None
    red = {"mean": "mean", "add": "sum", "sum": "sum", "min": "amin", "max": "amax"}[reduce]
    out = torch.zeros(uniq.numel(), dtype=edge_attr.dtype, device=edge_attr.device)
    return ei, out.scatter_reduce(0, inv, edge_attr, red, include_self=False)


def _isolated_edges(pos, is_out, k_isolated, batch):
    """New edges of the isolated nodes (data.py:506-524): ``(neighbors, distances)`` of the
    ``k_isolated`` nearest other nodes, column 0 of a ``k_isolated + 1`` search dropped."""
    r_max = float((pos.max(dim=0).values - pos.min(dim=0).values).norm())
    bq = batch[is_out] if batch is not None else None
    if not r_max > 0:                                   # one node, or all at one place: d < r_max never holds
        shape = (is_out.numel(), k_isolated)
        return (torch.full(shape, -1, dtype=torch.long, device=pos.device),
                torch.full(shape, -1.0, dtype=torch.float32, device=pos.device))
    if pos.is_cuda:
        from .neighbors import knn_2
        nb, d = knn_2(pos, pos[is_out], k_isolated + 1, r_max=r_max, batch_search=batch,
                      batch_query=bq)
    else:
        nb, d = _knn_isolated_torch(pos, pos[is_out], k_isolated + 1, r_max, batch, bq)
    return nb.view(-1, k_isolated + 1)[:, 1:].contiguous(), d.view(-1, k_isolated + 1)[:, 1:].contiguous()


def _partition_adjacency_torch(neighbor_index, neighbor_distance, k, w, pos, k_isolated, reduce,
                               batch):
    """The reference's composition step by step in torch (graph.py:77-94, data.py:490-561,
    utils/graph.py:466-502): the route of CPU tensors and of tables whose rows repeat a
    neighbour.  Duplicates are merged by a sort (``coalesce``), the regression line comes from
    the same five f64 sums as on the device."""
    N = neighbor_index.shape[0]
    dev = neighbor_index.device
    source = torch.arange(N, device=dev).repeat_interleave(k)
    target = neighbor_index[:, :k].flatten()
    mask = target >= 0
    source, target = source[mask], target[mask]
    if w > 0:
        distances = neighbor_distance[:, :k].flatten()[mask].float()
        mean = (distances.double().sum() / max(distances.numel(), 1)).float()
        edge_attr = 1 / (w + distances / mean)
    else:
        edge_attr = torch.ones_like(source, dtype=torch.float)
    if source.numel() == 0:
        edge_attr = None                                              # data.py:492-494
    linked = torch.zeros(N, dtype=torch.bool, device=dev)
    linked[source] = True
    linked[target] = True
    is_out = torch.where(~linked)[0]
    if k_isolated > 0 and is_out.numel() > 0:
        if pos is None:
            raise ValueError("isolated nodes need pos to be connected")
        nb, dist = _isolated_edges(pos, is_out, k_isolated, batch)
        new_s, new_t, dist = is_out.repeat_interleave(k_isolated), nb.flatten(), dist.flatten()
        found = new_t >= 0
        if edge_attr is not None:
            d = (pos[source] - pos[target]).float().norm(dim=1).double()
            wd = edge_attr.double()
            a, b = _regression_line(float(d.numel()), float(d.sum()), float((d * d).sum()),
                                    float(wd.sum()), float((d * wd).sum()))
            new_w = dist * torch.tensor(a, dtype=torch.float32, device=dev) \
                + torch.tensor(b, dtype=torch.float32, device=dev)
            edge_attr = torch.cat((edge_attr, new_w[found]))
        source, target = torch.cat((source, new_s[found])), torch.cat((target, new_t[found]))
    lo, hi = torch.minimum(source, target), torch.maximum(source, target)
    edge_index = torch.stack((lo, hi))
    if dev.type == "cuda" and edge_index.numel():
        from .shims.pyg_shim import coalesce
        edge_index, edge_attr = coalesce(edge_index, edge_attr, reduce=reduce)
    else:
        edge_index, edge_attr = _coalesce_torch(edge_index, edge_attr, reduce)
    keep = edge_index[0] != edge_index[1]
    edge_index = edge_index[:, keep]
    edge_attr = None if edge_attr is None else edge_attr[keep]
    csr = torch.zeros(N + 1, dtype=torch.long, device=dev)
    csr[1:] = torch.cumsum(torch.bincount(edge_index[0], minlength=N), 0)
    return PartitionGraph(edge_index, edge_attr, csr, is_out.numel())


def partition_adjacency(neighbor_index, neighbor_distance, k, w=-1, pos=None, k_isolated=1,
                        reduce="mean", batch=None):
    """The partition's input graph from the kNN table: ``AdjacencyGraph(k, w)`` ->
    ``ConnectIsolated(k_isolated)`` -> ``Data.to_trimmed(reduce)`` (src/transforms/graph.py:67-96,
    src/data/data.py:481-586, src/utils/graph.py:466-502) and the forward-star arrays of
    ``CutPursuitPartition._process`` (src/transforms/partition.py:190-196), in four kernel
    passes over the table (``csrc/adjacency.hip``) instead of an edge list, a ``unique``, a
    ``lstsq`` and a ``coalesce`` sort.

    ``neighbor_index`` [N, K] int64 (any negative entry = missing), ``neighbor_distance`` [N, K]
    f32 (may be None when ``w <= 0``); the first ``k <= K`` columns are read in place.  Edge
    weights are ``1 / (w + d / mean(d))`` or 1 (``w <= 0``).  Nodes that no directed edge touches
    get edges to their ``k_isolated`` nearest other nodes (``pos`` [N, 3] required then; ``batch``
    keeps the search within a cloud), weighted by the least-squares line of weight against
    end-point distance - closed form on five f64 sums, where the reference calls ``lstsq``.  Then
    edges are flipped to i < j, self loops dropped and both directions of a pair merged with
    ``reduce`` ('mean', 'add' / 'sum', 'min', 'max').  When the table holds no edge at all the
    graph has no ``edge_attr`` (data.py:492-494, 526-528).

    Returns a ``PartitionGraph``.  ``source_csr`` / ``edge_index[1]`` / identity restate what
    ``grid_graph.edge_list_to_forward_star`` returns for sorted input; that package is
    third-party and unpinned here.

    A table whose rows name a neighbour twice (oversampled neighbourhoods) cannot be trimmed by
    look-up: the kernels report it and the same result is computed through ``coalesce``, as it
    is for CPU tensors."""
    if reduce not in _REDUCE_CODES:
        raise ValueError(f"reduce must be one of {sorted(_REDUCE_CODES)}, got {reduce!r}")
    if neighbor_index.dim() != 2 or neighbor_index.dtype != torch.long:
        raise ValueError("neighbor_index must be an [N, K] int64 tensor")
    N, K = neighbor_index.shape
    k, k_isolated = int(k), int(k_isolated)
    if not 1 <= k <= K:
        raise ValueError(f"k must be in [1, {K}], got {k}")
    if k_isolated < 0:
        raise ValueError("k_isolated must be >= 0")
    w = float(w)
    if w > 0 and neighbor_distance is None:
        raise ValueError("w > 0 needs neighbor_distance")
    if neighbor_distance is not None and neighbor_distance.shape != neighbor_index.shape:
        raise ValueError("neighbor_distance must have neighbor_index's shape")
    args = (neighbor_index, neighbor_distance, k, w, pos, k_isolated, reduce, batch)
    if not neighbor_index.is_cuda:
        return _partition_adjacency_torch(*args)
    _lib.require_cuda(neighbor_distance, pos, batch)
    if k > 64 or k_isolated > 64:
        return _partition_adjacency_torch(*args)
    from .ops import _workspace
    L = _lib.lib
    dev = neighbor_index.device
    # the table is read where it lies: knn_1's result is columns 1 .. K of a [N, K + 1] search
    nn, dist = neighbor_index, None
    if w > 0:
        dist = neighbor_distance if neighbor_distance.dtype == torch.float32 else neighbor_distance.float()

    def pitched(t):
        return t is None or (t.stride(1) == 1 and t.stride(0) >= K) or N <= 1
    if not (pitched(nn) and pitched(dist) and (dist is None or N <= 1 or dist.stride(0) == nn.stride(0))):
        nn, dist = nn.contiguous(), None if dist is None else dist.contiguous()
    ld = max(int(nn.stride(0)), K) if N > 1 else K
    stream = _lib.stream_ptr(dev)

    # pass A: mean distance, linked flags, repeated-neighbour check, isolated count
    linked = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    nb_stats = L.spt_adjacency_stats_workspace_bytes(N)
    ws = _workspace(nb_stats, dev)
    with torch.cuda.device(dev):
        st = L.spt_adjacency_stats(_lib.ptr(nn), _lib.ptr(dist), N, ld, k, _lib.ptr(linked),
                                   _lib.ptr(stats), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(st, "spt_adjacency_stats")
    n_valid, sum_d, n_iso, flags = stats[:4].tolist()           # host sync (the reference's masks)
    n_valid, n_iso, flags = int(n_valid), int(n_iso), int(flags)
    if flags & 2:
        raise ValueError(f"neighbor_index holds entries >= N = {N}")
    if flags & 1:
        return _partition_adjacency_torch(*args)
    weighted = n_valid > 0
    mean = float(torch.tensor(sum_d / n_valid, dtype=torch.float64).float()) if (w > 0 and weighted) else 1.0

    iso_index = iso_nn = iso_w = None
    rows_iso = 0
    if k_isolated > 0 and n_iso > 0:
        if pos is None:
            raise ValueError("isolated nodes need pos to be connected")
        posf = pos.detach().float().contiguous()
        iso_index = torch.nonzero(linked[:N] == 0).view(-1)
        iso_nn, iso_d = _isolated_edges(posf, iso_index, k_isolated, batch)
        rows_iso = iso_index.numel()
        if weighted:
            sums = torch.empty(4, dtype=torch.float64, device=dev)
            ws = _workspace(nb_stats, dev)
            with torch.cuda.device(dev):
                st = L.spt_adjacency_regression(_lib.ptr(nn), _lib.ptr(dist), _lib.ptr(posf), N, ld,
                                                k, w, mean, _lib.ptr(sums), _lib.ptr(ws),
                                                ws.numel(), stream)
            _lib.check(st, "spt_adjacency_regression")
            a, b = _regression_line(float(n_valid), *sums.tolist())
            iso_w = (iso_d * torch.tensor(a, dtype=torch.float32, device=dev)
                     + torch.tensor(b, dtype=torch.float32, device=dev)).contiguous()   # data.py:556

    # pass B: surviving entries, counts per smaller end point, scan
    keep = torch.empty(max(N + rows_iso, 1), dtype=torch.int64, device=dev)
    row_start = torch.empty(N + 1, dtype=torch.int32, device=dev)
    ws = _workspace(L.spt_adjacency_count_workspace_bytes(N), dev)
    with torch.cuda.device(dev):
        st = L.spt_adjacency_count(_lib.ptr(nn), N, ld, k, _lib.ptr(linked), _lib.ptr(iso_index),
                                   _lib.ptr(iso_nn), rows_iso, k_isolated, _lib.ptr(keep),
                                   _lib.ptr(row_start), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(st, "spt_adjacency_count")
    E = int(row_start[N]) & 0xFFFFFFFF                            # host sync: output size

    # pass C: fill, per-row sort, emit
    edge_index = torch.empty((2, E), dtype=torch.int64, device=dev)
    edge_attr = torch.empty(E, dtype=torch.float32, device=dev) if weighted else None
    source_csr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    nbytes = L.spt_adjacency_fill_workspace_bytes(N, E)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_adjacency_fill(_lib.ptr(nn), _lib.ptr(dist), N, ld, k, w, mean, _lib.ptr(linked),
                                  _lib.ptr(iso_index), _lib.ptr(iso_nn), _lib.ptr(iso_w), rows_iso,
                                  k_isolated, _REDUCE_CODES[reduce], _lib.ptr(keep),
                                  _lib.ptr(row_start), E, _lib.ptr(edge_index), _lib.ptr(edge_attr),
                                  _lib.ptr(source_csr), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(st, "spt_adjacency_fill")
    return PartitionGraph(edge_index, edge_attr, source_csr, n_iso)
