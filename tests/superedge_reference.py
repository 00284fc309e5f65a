"""Plain-torch restatement of the superedge stage, step by step as the reference composes it:
``subedges`` (src/utils/graph.py:99-463 with ``edge_wise_points``, ``scatter_nearest_neighbor``,
``base_vectors_3d``, ``idx_preserving_mask``, ``sparse_sort``, ``scatter_pca``,
``sparse_sort_along_direction``) and ``_minimalistic_horizontal_edge_features``
(src/transforms/graph.py:950-1060), in a dtype of the caller's choice (f32 as the reference runs,
f64 as the yardstick of the feature tests).  For the tests only; pinned on the reference-made
fixtures by tests/test_superedges_reference_cpu.py.

Also here: the comparison the GPU tests and the CPU tests share (``compare_subedges``), and the
single-edge f64 keys and thresholds behind the one excuse the size-class test allows
(``edge_thresholds``).
"""
import torch


def to_trimmed(edge_index):
    lo, hi = torch.minimum(edge_index[0], edge_index[1]), torch.maximum(edge_index[0], edge_index[1])
    keep = lo != hi
    lo, hi = lo[keep], hi[keep]
    n = int(hi.max()) + 1 if hi.numel() else 1
    key = torch.unique(lo * n + hi, sorted=True)
    return torch.stack([key // n, key % n])


def base_vectors_3d(x):
    a = x.clone()
    a[a.norm(dim=1) == 0] = torch.tensor([1.0, 0.0, 0.0], dtype=x.dtype)
    a = a / a.norm(dim=1).view(-1, 1)
    b = torch.stack((a[:, 1] - a[:, 2], a[:, 2] - a[:, 0], a[:, 0] - a[:, 1]), dim=1)
    b[b.norm(dim=1) == 0] = torch.tensor([2.0, 1.0, -1.0], dtype=x.dtype)
    b = b / b.norm(dim=1).view(-1, 1)
    return torch.stack((a, b, torch.linalg.cross(a, b)), dim=1)


def _sum(x, uid, num):
    return torch.zeros((num,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, uid, x)


def _ext(x, uid, num, red):
    out = torch.zeros((num,) + tuple(x.shape[1:]), dtype=x.dtype)
    return out.scatter_reduce(0, uid.view([-1] + [1] * (x.dim() - 1)).expand_as(x), x, red,
                              include_self=False)


def _argmin(value, uid, num):
    at = torch.arange(value.numel())
    at = torch.where(value == _ext(value, uid, num, "amin")[uid], at, torch.full_like(at, value.numel()))
    return _ext(at, uid, num, "amin")


def _expand(points, index, seg, num_segments):
    """Points of segment ``seg[e]`` for every e, in ascending point order: (rows, ids, e)."""
    order = torch.argsort(index, stable=True)
    size = torch.bincount(index, minlength=num_segments)
    start = torch.cumsum(size, 0) - size
    sz = size[seg]
    uid = torch.repeat_interleave(torch.arange(seg.numel()), sz)
    first = torch.cumsum(sz, 0) - sz
    pid = order[start[seg][uid] + torch.arange(int(sz.sum())) - first[uid]]
    return points[pid], pid, uid


def _group_sort(value, group, descending=False):
    p1 = torch.argsort(value, descending=descending, stable=True)
    return p1[torch.argsort(group[p1], stable=True)]


def pair_anchors(points, index, edge_index, cycles, num_segments):
    E = edge_index.shape[1]
    cnt = torch.bincount(index, minlength=num_segments).clamp(min=1).view(-1, 1)
    centroid = (_sum(points.double(), index, num_segments) / cnt).to(points.dtype)
    S_pts, S_idx, S_uid = _expand(points, index, edge_index[0], num_segments)
    T_pts, T_idx, T_uid = _expand(points, index, edge_index[1], num_segments)
    sc = centroid[edge_index[0]]
    si = ti = None
    for _ in range(int(cycles)):
        ti = T_idx[_argmin((T_pts - sc[T_uid]).norm(dim=1), T_uid, E)]
        si = S_idx[_argmin((S_pts - points[ti][S_uid]).norm(dim=1), S_uid, E)]
        sc = points[si]
    return torch.stack((si, ti))


def _first_component(P, uid, num):
    x = P.double()
    cnt = torch.bincount(uid, minlength=num).clamp(min=1).view(-1, 1).double()
    d = x - (_sum(x, uid, num) / cnt)[uid]
    cov = _sum(d.unsqueeze(2) * d.unsqueeze(1), uid, num) / cnt.view(-1, 1, 1)
    return torch.linalg.eigh(cov)[1][:, :, -1].to(P.dtype)


def subedges_reference(pos, index, edge_index, ratio=0.2, k_min=20, cycles=3, margin=0.2,
                       halfspace_filter=True, bbox_filter=True, target_pc_flip=True,
                       source_pc_sort=False, dtype=torch.float32, anchors=None):
    """``(edge_index trimmed, pairs [2, M], uid [M], anchors [2, E])``."""
    points = pos.detach().cpu().to(dtype)
    index = index.cpu().long()
    edge_index = to_trimmed(edge_index.cpu().long())
    E = edge_index.shape[1]
    z = torch.empty(0, dtype=torch.long)
    if E == 0:
        return edge_index, torch.stack([z, z]), z, torch.stack([z, z])
    S = int(index.max()) + 1
    if anchors is None:
        anchors = pair_anchors(points, index, edge_index, cycles, S)
    s_anchor, t_anchor = points[anchors[0]], points[anchors[1]]
    base = base_vectors_3d(t_anchor - s_anchor)
    S_pts, S_idx, S_uid = _expand(points, index, edge_index[0], S)
    T_pts, T_idx, T_uid = _expand(points, index, edge_index[1], S)

    def project(X, uid, anchor):
        d, b = X - anchor[uid], base[uid]
        return torch.stack([(d[:, 0] * b[:, k, 0] + d[:, 1] * b[:, k, 1]) + d[:, 2] * b[:, k, 2]
                            for k in range(3)], dim=1)

    S_pts, T_pts = project(S_pts, S_uid, s_anchor), project(T_pts, T_uid, t_anchor)

    def take(mask, P, I, U):
        keep = torch.where(mask | (_sum(mask.long(), U, E) == 0)[U])[0]
        return P[keep], I[keep], U[keep]

    if halfspace_filter:
        S_pts, S_idx, S_uid = take(S_pts[:, 0] <= margin, S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(T_pts[:, 0] >= -margin, T_pts, T_idx, T_uid)
    if bbox_filter:
        st_min = torch.max(_ext(S_pts[:, 1:], S_uid, E, "amin"),
                           _ext(T_pts[:, 1:], T_uid, E, "amin")).clamp(max=-margin)
        st_max = torch.min(_ext(S_pts[:, 1:], S_uid, E, "amax"),
                           _ext(T_pts[:, 1:], T_uid, E, "amax")).clamp(min=margin)

        def inside(P, U):
            return (P[:, 1:] >= st_min[U]).all(dim=1) & (P[:, 1:] <= st_max[U]).all(dim=1)
        S_pts, S_idx, S_uid = take(inside(S_pts, S_uid), S_pts, S_idx, S_uid)
        T_pts, T_idx, T_uid = take(inside(T_pts, T_uid), T_pts, T_idx, T_uid)

    p = _group_sort(S_pts[:, 0], S_uid, descending=True)
    S_pts, S_idx, S_uid = S_pts[p], S_idx[p], S_uid[p]
    p = _group_sort(T_pts[:, 0], T_uid)
    T_pts, T_idx, T_uid = T_pts[p], T_idx[p], T_uid[p]

    s_size, t_size = torch.bincount(S_uid, minlength=E), torch.bincount(T_uid, minlength=E)
    r32 = torch.tensor(ratio, dtype=torch.float32)                 # torch's f32 `size * ratio`
    s_k = (s_size.float() * r32).long().clamp(min=k_min).min(s_size)
    t_k = (t_size.float() * r32).long().clamp(min=k_min).min(t_size)
    st_k = torch.min(s_k, t_k)

    def head(size):
        first = torch.cumsum(size, 0) - size
        grp = torch.repeat_interleave(torch.arange(E), st_k)
        return first[grp] + torch.arange(int(st_k.sum())) - (torch.cumsum(st_k, 0) - st_k)[grp]

    sel = head(s_size)
    S_pts, S_idx, S_uid = S_pts[sel], S_idx[sel], S_uid[sel]
    sel = head(t_size)
    T_pts, T_idx, T_uid = T_pts[sel], T_idx[sel], T_uid[sel]

    s_v, t_v = _first_component(S_pts, S_uid, E), _first_component(T_pts, T_uid, E)
    kk = st_k.view(-1, 1)

    def mean_of(P, U):
        return (_sum(P.double(), U, E) / kk).to(P.dtype)

    if target_pc_flip and not source_pc_sort:
        t_minp = T_pts[_argmin((T_pts * t_v[T_uid]).sum(dim=1), T_uid, E)]
        st_u = t_minp - mean_of(S_pts, S_uid)
        st_u = st_u / st_u.norm(dim=1).view(-1, 1)
        flip = (s_v * t_v).sum(dim=1) <= (s_v * st_u).sum(dim=1)
        t_v = torch.where(flip.view(-1, 1), -t_v, t_v)
    elif source_pc_sort:
        t_v = s_v

    def along(P, I, U, v):
        q = _group_sort(((P - mean_of(P, U)[U]) * v[U]).sum(dim=1), U)
        return I[q], U[q]

    S_idx, S_uid = along(S_pts, S_idx, S_uid, s_v)
    T_idx, T_uid = along(T_pts, T_idx, T_uid, t_v)
    return edge_index, torch.vstack((S_idx, T_idx)), S_uid, anchors


def edge_features_reference(pos, pairs, uid, num_edges, dtype=torch.float64):
    """The 7 features in closed form from given pairs (graph.py:1008-1058), unclipped std kept
    clipped as the reference stores it."""
    E = int(num_edges)
    p = pos.detach().cpu().to(dtype)
    pairs, uid = pairs.cpu().long(), uid.cpu().long()
    offset = p[pairs[1]] - p[pairs[0]]
    cnt = torch.bincount(uid, minlength=E).clamp(min=1).to(dtype).view(-1, 1)
    mean_off = _sum(offset, uid, E) / cnt
    base = base_vectors_3d(mean_off)[uid]
    uvw = torch.stack([(offset * base[:, k]).sum(dim=1) for k in range(3)], dim=1)
    dev = uvw - (_sum(uvw, uid, E) / cnt)[uid]
    std = (_sum(dev * dev, uid, E) / ((cnt - 1).clamp(min=1) + 1e-6)).sqrt().clip(-2, 2)
    mean_dist = (_sum(offset.norm(dim=1).view(-1, 1), uid, E) / cnt).sqrt()
    return torch.cat((mean_off, std, mean_dist), dim=1)


def per_edge(pairs, uid, E):
    pairs, uid = pairs.cpu(), uid.cpu()
    first = torch.searchsorted(uid, torch.arange(E + 1))
    return [(pairs[0, first[e]:first[e + 1]].tolist(), pairs[1, first[e]:first[e + 1]].tolist())
            for e in range(E)]


def compare_subedges(got, ref, allow=None):
    """``got`` / ``ref`` = (edge_index, pairs, uid).  Edge list and uid exact, the selected point
    SETS of every edge exact, the pairing equal up to the target-side reversal (the sign of the
    eigenvectors, tests/test_subedges.py) on at most a third of the edges.  ``allow(e)``, when
    given, is asked about an edge whose sets differ; it returns True to excuse the edge.
    Returns ``(same [E] bool: pairing identical to ref's, excused edge ids)``."""
    ei, pairs, uid = (t.cpu() for t in got)
    r_ei, r_pairs, r_uid = (t.cpu() for t in ref)
    assert torch.equal(ei, r_ei)
    E = ei.shape[1]
    a, b = per_edge(pairs, uid, E), per_edge(r_pairs, r_uid, E)
    same = torch.zeros(E, dtype=torch.bool)
    excused, reversed_ = [], 0
    for e, ((s, t), (rs, rt)) in enumerate(zip(a, b)):
        if sorted(s) != sorted(rs) or sorted(t) != sorted(rt):
            assert allow is not None and allow(e, s, t, rs, rt), f"edge {e}: selected sets differ"
            excused.append(e)
            continue
        direct = list(zip(s, t)) == list(zip(rs, rt)) or list(zip(s[::-1], t[::-1])) == list(zip(rs, rt))
        flipped = list(zip(s, t[::-1])) == list(zip(rs, rt)) or list(zip(s[::-1], t)) == list(zip(rs, rt))
        assert direct or flipped, f"edge {e}: pairing is neither the reference's nor its reversal"
        same[e] = direct
        reversed_ += int(not direct)
    if not excused:
        assert torch.equal(uid, r_uid)
    assert reversed_ <= E // 3, f"{reversed_} of {E} edges paired in the other direction"
    return same, excused


def edge_thresholds(pos, index, s, t, a_s, a_t, ratio, k_min, margin, halfspace_filter=True,
                    bbox_filter=True):
    """f64 keys of one edge (source segment ``s``, target ``t``, anchors ``a_s`` / ``a_t``):
    ``{point id: smallest distance of one of its keys to the threshold that decides it}`` over
    both sides - the margin, the four box bounds, and the first-coordinate keys on either side of
    rank ``st_k``."""
    p = pos.detach().cpu().double()
    index = index.cpu().long()
    base = base_vectors_3d((p[a_t] - p[a_s]).view(1, 3))[0]
    sides = []
    for seg, anchor in ((s, a_s), (t, a_t)):
        ids = torch.where(index == seg)[0]
        sides.append((ids, (p[ids] - p[anchor]) @ base.t()))
    near = {}
    alive = []
    for sd, (ids, X) in enumerate(sides):
        m = X[:, 0] <= margin if sd == 0 else X[:, 0] >= -margin
        if not halfspace_filter or not m.any():
            m = torch.ones_like(m)
        d = (X[:, 0] - (margin if sd == 0 else -margin)).abs()
        for i, q in enumerate(ids.tolist()):
            near[q] = float(d[i]) if halfspace_filter else float("inf")
        alive.append(m)
    if bbox_filter:
        lo = torch.max(sides[0][1][alive[0], 1:].min(0).values,
                       sides[1][1][alive[1], 1:].min(0).values).clamp(max=-margin)
        hi = torch.min(sides[0][1][alive[0], 1:].max(0).values,
                       sides[1][1][alive[1], 1:].max(0).values).clamp(min=margin)
        for sd, (ids, X) in enumerate(sides):
            d = torch.minimum((X[:, 1:] - lo).abs().min(1).values, (X[:, 1:] - hi).abs().min(1).values)
            m = ((X[:, 1:] >= lo) & (X[:, 1:] <= hi)).all(1) & alive[sd]
            if m.any():
                alive[sd] = m
            for i, q in enumerate(ids.tolist()):
                near[q] = min(near[q], float(d[i]))
    r32 = torch.tensor(ratio, dtype=torch.float32)
    ks = []
    for m in alive:
        n = int(m.sum())
        ks.append(min(max(int((torch.tensor(float(n), dtype=torch.float32) * r32).long()), k_min), n))
    st_k = min(ks)
    for sd, (ids, X) in enumerate(sides):
        key = torch.sort(X[alive[sd], 0], descending=(sd == 0)).values
        cut = [key[st_k - 1]] + ([key[st_k]] if st_k < key.numel() else [])
        for i, q in enumerate(ids.tolist()):
            near[q] = min(near[q], min(float((X[i, 0] - c).abs()) for c in cut))
    return near
