"""From logits back to the cloud, on the kernels of ``csrc/predict.hip``: the pieces that
``SemanticSegmentationOutput`` (src/utils/output_semantic.py) and the multi-run inference of
src/models/semantic.py:485-616 are made of.

``row_argmax``        ``torch.argmax(logits, dim=1)`` and the reference's ``void_mask``;
``accumulate_rows_``  ``acc[node_id] += src`` of one inference run, with the run stamp whose
                      non-zero entries are the reference's ``seen``;
``labels_through``    labels carried down one or two hops of the hierarchy
                      (``pred[super_index_0][super_index_raw]``), each hop an index tensor or a
                      ``data.Cluster`` taken as it is stored - no ``to_super_index()`` - with the
                      confusion matrix against per-point labels fused in.

Every result is an integer, a boolean or an f32 formed by one add per element: equal to the
reference's bit for bit.

Host reads: none with ``check=False`` (an inference graph can capture the calls); with
``check=True`` one read of the status record at the end of the call, which raises ``ValueError``
naming what was out of range.  The device results of a failed check are still defined: an index
out of range gives the label -1, a point out of range is not written.

CPU tensors take a torch composition of the same rules, with the same results and errors."""
import torch

from . import _lib

__all__ = ["row_argmax", "void_mask", "accumulate_rows_", "labels_through", "MAX_CLASSES"]

MAX_CLASSES = 32        # of the fused confusion matrix (as ops.histogram_confusion_matrix)


def _is_cluster(hop):
    return hasattr(hop, "pointers") and hasattr(hop, "points")


def _check_logits(logits):
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"logits must be [rows, C >= 1], got {tuple(logits.shape)}")


def _check_hist(hist, rows=None):
    if hist.dim() != 2 or hist.shape[1] < 1 or hist.is_floating_point():
        raise ValueError("hist must be an integer [rows, ncols >= 1] tensor")
    if rows is not None and hist.shape[0] != rows:
        raise ValueError(f"hist holds {hist.shape[0]} rows for {rows} rows of logits")


def _void_torch(hist):
    return hist[:, -1] / hist.sum(dim=1) > 0.5


def _row_argmax_device(logits, hist):
    src = logits if logits is not None else hist
    dev, rows = src.device, src.shape[0]
    pred = is_void = None
    c = ncols = 0
    if logits is not None:
        logits = logits.detach().contiguous()
        c = logits.shape[1]
        pred = torch.empty(rows, dtype=torch.int64, device=dev)
    if hist is not None:
        _lib.require_cuda(hist)
        hist = hist.detach().long().contiguous()
        ncols = hist.shape[1]
        is_void = torch.empty(rows, dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_row_argmax_f32(_lib.ptr(logits), rows, c, _lib.ptr(hist), ncols,
                                         _lib.ptr(pred), _lib.ptr(is_void), _lib.stream_ptr(dev))
    _lib.check(st, "spt_row_argmax_f32")
    return pred, is_void


def row_argmax(logits, hist=None):
    """``torch.argmax(logits, dim=1)`` of f32 ``[rows, C]`` logits: the first maximum, a NaN above
    every number, the first NaN.  With ``hist`` (int ``[rows, ncols]``, void counts in the last
    column) returns ``(pred, void_mask)``, the mask as ``void_mask`` below, from the same launch.
    Logits that are not f32 take ``torch.argmax``."""
    _check_logits(logits)
    if hist is not None:
        _check_hist(hist, logits.shape[0])
    if not logits.is_cuda or logits.dtype != torch.float32:
        pred = torch.argmax(logits, dim=1)
        return pred if hist is None else (pred, void_mask(hist))
    pred, is_void = _row_argmax_device(logits, hist)
    return pred if hist is None else (pred, is_void)


def void_mask(hist):
    """``SemanticSegmentationOutput.void_mask`` of a label histogram: ``void / total > 0.5`` with
    both integers converted to f32 and divided in f32, as torch's true division does (an empty
    row is 0 / 0 = NaN: not void)."""
    _check_hist(hist)
    if not hist.is_cuda:
        return _void_torch(hist)
    return _row_argmax_device(None, hist)[1]


def _check_accumulate(acc, src, node_id, stamp, run):
    if acc.dim() != 2 or src.dim() != 2 or acc.shape[1] != src.shape[1] or acc.shape[1] < 1:
        raise ValueError(f"acc [N, C] and src [n, C] must share C >= 1, got {tuple(acc.shape)} "
                         f"and {tuple(src.shape)}")
    if acc.dtype != torch.float32 or src.dtype != torch.float32:
        raise ValueError("acc and src must be float32")
    if node_id.dim() != 1 or node_id.numel() != src.shape[0] or node_id.is_floating_point():
        raise ValueError("node_id must hold one integer id per row of src")
    if stamp.dtype != torch.int32 or stamp.dim() != 1 or stamp.numel() != acc.shape[0]:
        raise ValueError("stamp must be an int32 tensor with one entry per row of acc")
    if not acc.is_contiguous() or not stamp.is_contiguous():
        raise ValueError("acc and stamp are written in place: they must be contiguous")
    if int(run) < 1:
        raise ValueError("run >= 1 (0 is the stamp of a row never written)")


def _raise_accumulate(dup, oob, run, n_rows):
    msgs = []
    if dup:
        msgs.append(f"{dup} node id(s) occur more than once in run {run}")
    if oob:
        msgs.append(f"{oob} node id(s) lie outside [0, {n_rows})")
    if msgs:
        raise ValueError("accumulate_rows_: " + "; ".join(msgs))


def accumulate_rows_(acc, src, node_id, stamp, run, check=True):
    """``acc[node_id] += src`` in place (f32 ``[N, C]`` and ``[n, C]``): one add per element, the
    reference's ``index_put_`` result bit for bit for unique ids.  ``stamp`` (int32 ``[N]``, zero
    before the first run) takes ``run`` (>= 1) at every row written: ``stamp != 0`` is ``seen``.
    An id that occurs twice in one run is added once and reported, an id outside ``[0, N)`` writes
    nothing and is reported - by ``ValueError`` under ``check=True`` (one host read), not at all
    under ``check=False``.  Returns ``acc``."""
    _check_accumulate(acc, src, node_id, stamp, run)
    run, n_rows = int(run), acc.shape[0]
    if not acc.is_cuda:
        ids = node_id.long()
        ok = (ids >= 0) & (ids < n_rows)
        rows = torch.where(ok)[0]
        uniq, inv = torch.unique(ids[rows], return_inverse=True)
        first = torch.full((uniq.numel(),), ids.numel(), dtype=torch.int64)
        first.scatter_reduce_(0, inv, rows, "amin", include_self=True)
        acc[uniq] = acc[uniq] + src[first]
        stamp[uniq] = run
        if check:
            _raise_accumulate(rows.numel() - uniq.numel(), ids.numel() - rows.numel(), run, n_rows)
        return acc
    _lib.require_cuda(src, node_id, stamp)
    dev = acc.device
    src = src.detach().contiguous()
    ids = node_id.detach().long().contiguous()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_rows_accumulate_f32(_lib.ptr(acc), n_rows, _lib.ptr(src), _lib.ptr(ids),
                                              ids.numel(), acc.shape[1], _lib.ptr(stamp), run,
                                              _lib.ptr(status), _lib.stream_ptr(dev))
    _lib.check(st, "spt_rows_accumulate_f32")
    if check:
        dup, oob = status.tolist()                                  # the host read
        _raise_accumulate(dup, oob, run, n_rows)
    return acc


# ------------------------------------------------------------------------------------------------
def _hop_sizes(hop):
    """(entries of the coarse side the hop must find, entries of the fine side it produces)."""
    if _is_cluster(hop):
        return hop.pointers.numel() - 1, hop.points.numel()
    return None, hop.numel()


def _index_torch(label, idx):
    ok = (idx >= 0) & (idx < label.numel())
    out = torch.full_like(idx, -1)
    out[ok] = label[idx[ok]]
    return out, int((~ok).sum())


def _cluster_torch(label, cluster):
    """The kernel's rules position by position: (labels [num_points] with -1 where nothing was
    written, point faults, pointer faults)."""
    ptr, pts = cluster.pointers.long(), cluster.points.long()
    nc, m = ptr.numel() - 1, pts.numel()
    out = torch.full((m,), -1, dtype=torch.int64)
    bad_ptr = int((ptr[1:] < ptr[:-1]).sum()) + int(bool(ptr[0] != 0) or bool(ptr[-1] != m))
    if m == 0 or nc == 0:
        return out, 0, bad_ptr
    j = torch.arange(m)
    v = (torch.searchsorted(ptr, j, right=True) - 1).clamp(0, nc - 1)
    claimed = (ptr[v] <= j) & (j < ptr[v + 1])
    in_range = (pts >= 0) & (pts < m)
    write = claimed & in_range
    out[pts[write]] = label[v[write]]
    return out, int((claimed & ~in_range).sum()), bad_ptr


_FAULTS = {
    "index": "hop {k}: {n} index entries outside [0, {bound})",
    "points": "hop {k}: {n} point(s) of the Cluster outside [0, {bound})",
    "pointers": "hop {k}: the Cluster's pointers are not a monotone 0 .. {bound} sequence "
                "({n} fault(s))",
}


def _raise_faults(faults):
    """faults: (hop number, kind, count, bound)."""
    msgs = [_FAULTS[kind].format(k=k, n=n, bound=bound) for k, kind, n, bound in faults if n]
    if msgs:
        raise ValueError("labels_through: " + "; ".join(msgs))


def _by_index(label, idx_a, idx_b, want_a, want_b, target, c, confmat, status):
    dev = label.device
    n_a, n_b = idx_a.numel(), 0 if idx_b is None else idx_b.numel()
    out_a = torch.empty(n_a, dtype=torch.int64, device=dev) if want_a else None
    out_b = torch.empty(n_b, dtype=torch.int64, device=dev) if want_b else None
    with torch.cuda.device(dev):
        st = _lib.lib.spt_labels_by_index_i64(
            _lib.ptr(label), label.numel(), _lib.ptr(idx_a), n_a, _lib.ptr(idx_b), n_b,
            _lib.ptr(out_a), _lib.ptr(out_b), _lib.ptr(target), c, _lib.ptr(confmat),
            _lib.ptr(status), _lib.stream_ptr(dev))
    _lib.check(st, "spt_labels_by_index_i64")
    return out_a, out_b


def _by_cluster(label, idx_a, cluster, want, target, c, confmat, status):
    dev = label.device
    ptr, pts = cluster.pointers, cluster.points
    m = pts.numel()
    out = torch.empty(m, dtype=torch.int64, device=dev) if want else None
    with torch.cuda.device(dev):
        st = _lib.lib.spt_labels_by_cluster_i64(
            _lib.ptr(label), label.numel(), _lib.ptr(idx_a), _lib.ptr(ptr), _lib.ptr(pts),
            ptr.numel() - 1, m, _lib.ptr(out), _lib.ptr(target), c, _lib.ptr(confmat),
            _lib.ptr(status), _lib.stream_ptr(dev))
    _lib.check(st, "spt_labels_by_cluster_i64")
    return out


def _prepare_hop(hop, dev):
    if _is_cluster(hop):
        if hop.pointers.device != dev or hop.points.device != dev:
            raise ValueError(f"a hop lives on {hop.pointers.device}, the labels on {dev}")
        if hop.pointers.dtype != torch.int64 or not hop.pointers.is_contiguous() \
                or hop.points.dtype != torch.int64 or not hop.points.is_contiguous():
            from .data import Cluster
            return Cluster(hop.pointers, hop.points)
        return hop
    if hop.dim() != 1 or hop.is_floating_point():
        raise ValueError("an index hop must be a 1-D integer tensor")
    if hop.device != dev:
        raise ValueError(f"a hop lives on {hop.device}, the labels on {dev}")
    return hop.detach().long().contiguous()


def labels_through(label, hops, target=None, num_classes=None, confmat=None,
                   want=("voxel", "raw"), check=True):
    """Carry ``label`` (int ``[n]``: one label per node of the coarsest level, typically
    ``row_argmax`` of the level-1 logits) down ``hops``, one or two of them, coarse to fine.  A
    hop is the finer level's ``super_index`` (int ``[n_fine]``) or the coarser level's ``sub``
    (a ``data.Cluster``), taken as stored.  The labels after the first hop are called
    ``'voxel'``, those after the second ``'raw'``; ``want`` says which to materialise.

    ``target`` (int labels of the FINEST level reached, anything outside ``[0, num_classes)`` is
    void) adds ``'confmat'``: the int64 ``[num_classes, num_classes]`` matrix ``[true,
    predicted]``, accumulated into ``confmat`` when given (``num_classes <= 32`` on the device).
    With ``want=()`` nothing of the finest level's size is written: the evaluation case.

    Launches on the device: index + index one, index + Cluster one (two when ``'voxel'`` is
    wanted too), Cluster + index and Cluster + Cluster two.  Returns a dict with the keys asked
    for.  ``check``: module docstring."""
    hops = list(hops) if isinstance(hops, (list, tuple)) else [hops]
    if len(hops) not in (1, 2):
        raise ValueError("labels_through takes one or two hops")
    want = (want,) if isinstance(want, str) else tuple(want)
    names = ("voxel", "raw")[:len(hops)]
    if any(w not in ("voxel", "raw") for w in want):
        raise ValueError(f"want holds names out of ('voxel', 'raw'): {want}")
    want = tuple(w for w in names if w in want)
    if label.dim() != 1 or label.is_floating_point():
        raise ValueError("label must be a 1-D integer tensor")
    dev = label.device
    hops = [_prepare_hop(h, dev) for h in hops]
    sizes = [label.numel()]
    for k, hop in enumerate(hops):
        coarse, fine = _hop_sizes(hop)
        if coarse is not None and coarse != sizes[-1]:
            raise ValueError(f"hop {k + 1} is a Cluster of {coarse} clusters over a level of "
                             f"{sizes[-1]} nodes")
        sizes.append(fine)
    c = 0
    if target is not None:
        if num_classes is None:
            raise ValueError("a target needs num_classes")
        c = int(num_classes)
        if c < 1:
            raise ValueError("num_classes must be positive")
        if target.dim() != 1 or target.is_floating_point() or target.numel() != sizes[-1]:
            raise ValueError(f"target must hold one integer label per node of the finest level "
                             f"({sizes[-1]}), got {tuple(target.shape)}")
        if target.device != dev:
            raise ValueError(f"target lives on {target.device}, the labels on {dev}")
        if confmat is None:
            confmat = torch.zeros(c, c, dtype=torch.int64, device=dev)
        elif confmat.dtype != torch.int64 or tuple(confmat.shape) != (c, c) \
                or not confmat.is_contiguous() or confmat.device != dev:
            raise ValueError(f"confmat must be a contiguous int64 [{c}, {c}] tensor on {dev}")
        target = target.detach().long().contiguous()
    elif confmat is not None:
        raise ValueError("confmat needs a target")
    if not want and target is None:
        raise ValueError("nothing to compute: want is empty and there is no target")
    label = label.detach().long().contiguous()
    if len(hops) == 2 and "raw" not in want and target is None:
        hops, sizes = hops[:1], sizes[:2]           # the second hop has nothing to produce

    if not label.is_cuda:
        return _labels_through_torch(label, hops, target, c, confmat, want, check, sizes)
    if c > MAX_CLASSES:
        raise ValueError(f"the fused confusion matrix holds at most {MAX_CLASSES} classes on the "
                         f"device, got {c}")

    status = torch.zeros((2, 4), dtype=torch.int32, device=dev)
    words = []                      # (launch, status word, hop number, kind of fault, bound)

    def cluster_words(launch, k):
        return [(launch, 1, k, "points", sizes[k]), (launch, 2, k, "pointers", sizes[k])]

    voxel = raw = None
    h1 = hops[0]
    last = len(hops) == 1
    if last or _is_cluster(h1):
        # the first hop on its own (with the matrix when it is the only one)
        if _is_cluster(h1):
            voxel = _by_cluster(label, None, h1, not last or "voxel" in want,
                                target if last else None, c if last else 0,
                                confmat if last else None, status[0])
            words += cluster_words(0, 1)
        else:
            voxel = _by_index(label, h1, None, "voxel" in want, False, target, c, confmat,
                              status[0])[0]
            words.append((0, 0, 1, "index", sizes[0]))
        if not last:
            h2 = hops[1]
            if _is_cluster(h2):
                raw = _by_cluster(voxel, None, h2, "raw" in want, target, c, confmat, status[1])
                words += cluster_words(1, 2)
            else:
                raw = _by_index(voxel, h2, None, "raw" in want, False, target, c, confmat,
                                status[1])[0]
                words.append((1, 0, 2, "index", sizes[1]))
    else:
        h2 = hops[1]
        words.append((0, 0, 1, "index", sizes[0]))
        if _is_cluster(h2):
            raw = _by_cluster(label, h1, h2, "raw" in want, target, c, confmat, status[0])
            words += cluster_words(0, 2)
            if "voxel" in want:     # (the same first hop again: its faults are counted above)
                voxel = _by_index(label, h1, None, True, False, None, 0, None, status[1])[0]
        else:
            voxel, raw = _by_index(label, h1, h2, "voxel" in want, "raw" in want, target, c,
                                   confmat, status[0])
            words.append((0, 1, 2, "index", sizes[1]))
    out = {}
    if "voxel" in want:
        out["voxel"] = voxel
    if "raw" in want:
        out["raw"] = raw
    if target is not None:
        out["confmat"] = confmat
    if check:
        counts = status.tolist()                                    # the host read
        _raise_faults([(k, kind, counts[launch][word], bound)
                       for launch, word, k, kind, bound in words])
    return out


def _labels_through_torch(label, hops, target, c, confmat, want, check, sizes):
    """The same rules as a torch composition, for CPU tensors."""
    faults, levels, cur = [], [], label
    for k, hop in enumerate(hops, start=1):
        if _is_cluster(hop):
            cur, bad_points, bad_ptr = _cluster_torch(cur, hop)
            faults += [(k, "points", bad_points, sizes[k]), (k, "pointers", bad_ptr, sizes[k])]
        else:
            cur, bad = _index_torch(cur, hop)
            faults.append((k, "index", bad, sizes[k - 1]))
        levels.append(cur)
    out = {name: lv for name, lv in zip(("voxel", "raw"), levels) if name in want}
    if target is not None:
        fin = levels[-1]
        ok = (target >= 0) & (target < c) & (fin >= 0) & (fin < c)
        confmat.view(-1).index_add_(0, target.clamp(0, c - 1) * c + fin.clamp(0, c - 1), ok.long())
        out["confmat"] = confmat
    if check:
        _raise_faults(faults)
    return out
