"""Panoptic evaluation on the kernels of ``csrc/panoptic.hip``: what stands between an instance
prediction and a Panoptic Quality in the reference's ``validation_step`` / ``test_step``
(src/models/panoptic.py:1066-1073, 1125).

``merge_instances``      ``InstanceData.merge`` (src/data/instance.py:227-253): level-1 overlaps
                         merged into the predicted instances;
``pair_stats``           ``iou_and_size`` + ``search_void`` per pair, and what
                         ``remove_void(C)[0].iou_and_size()`` gives without compacting anything;
``panoptic_counts_``     the five ``[C]`` counters ``PanopticQuality3D.compute``
                         (src/metrics/panoptic.py:225-323) is made of, added into a device state;
``weighted_group_mean``  ``scatter_mean_weighted`` (src/utils/scatter.py:17-38);
``major_objects``        ``InstanceData.major`` (src/data/instance.py:162-225), the target object
                         of each cluster in the edge-affinity loss, without a host read.

Integer results are exact; ``iou`` is one correctly rounded f32 division of the two converted
integers, as torch divides int64 tensors; the weighted mean equals the reference's CPU result
bit for bit for groups of up to ``SEQUENTIAL_ROWS`` rows.

Host reads on the device: ``merge_instances`` two (the key extents, then the record holding the
number of merged pairs and the fault counts); ``pair_stats``, ``panoptic_counts_`` and
``weighted_group_mean(check=False)`` none - faults are counted in status records that the caller
reads when it wants to know (``PanopticQuality3D.compute`` reads them with the state).

CPU tensors take a torch composition of the same rules, with the same results and errors."""
from types import SimpleNamespace

import torch

from . import _lib
from .instance import InstanceData, _consecutive

__all__ = ["merge_instances", "pair_stats", "panoptic_counts_", "weighted_group_mean",
           "semantic_score", "major_objects", "verify_major",
           "new_state", "state_views", "MAX_CLASSES", "SEQUENTIAL_ROWS", "STATUS_WORDS"]

MAX_CLASSES = 32          # of the per-workgroup tables of panoptic_counts_ on the device
SEQUENTIAL_ROWS = 512     # weighted_group_mean: groups up to this are summed by one lane, in order
MAX_ITEMS = 2 ** 31 - 2   # pairs, clusters, rows
STATUS_WORDS = 4          # pointers faults, obj outside the key range, predictions out of range,
#                           IoUs outside [0, 1]

_FAULTS = ("{n} fault(s) of pointers (not a monotone 0 .. num_pairs sequence)",
           "{n} object id(s) outside the range the key was built for",
           "{n} prediction(s) of non-void clusters outside [0, num_classes)",
           "{n} pair(s) with an IoU outside [0, 1] (an empty union)")


def raise_status(who, words):
    msgs = [_FAULTS[k].format(n=n) for k, n in enumerate(words) if n]
    if msgs:
        raise ValueError(f"{who}: " + "; ".join(msgs))


def _bits_for(n):
    """Bits of a field holding ``n`` values (at least one)."""
    return max(1, (int(n) - 1).bit_length())


def _check_data(d):
    if d.num_items > MAX_ITEMS or d.num_groups > MAX_ITEMS:
        raise ValueError(f"at most {MAX_ITEMS} pairs and clusters")


def _workspace(nbytes, dev):
    from . import ops
    return ops._workspace(nbytes, dev)


# ------------------------------------------------------------------------------------------------
def _merge_checks(data, idx, num_parents):
    if idx.shape != torch.Size([data.num_groups]):
        raise AssertionError(
            f"Expected indices of shape {torch.Size([data.num_groups])}, but received shape "
            f"{idx.shape} instead")
    if idx.is_floating_point():
        raise ValueError("idx must be an integer tensor")
    if idx.device != data.device:
        raise ValueError(f"idx lives on {idx.device}, the instance data on {data.device}")
    if data.num_items == 0:                                        # sparse.py:27
        raise AssertionError("At least one group index is required.")
    if num_parents is not None and not 1 <= int(num_parents) <= data.num_groups:
        raise ValueError(f"num_parents must lie in 1 .. {data.num_groups}, got {num_parents}")
    _check_data(data)


def _merge_layout(obj_min, obj_max, idx_min, idx_max, num_parents):
    """(num_parents, obj_bits) from the extents; the refusals both routes share."""
    if num_parents is None:
        num_parents = idx_max + 1
    if idx_min != 0 or idx_max != num_parents - 1:
        raise AssertionError(f"Expected contiguous indices in [0, max]: got [{idx_min}, "
                             f"{idx_max}] for {num_parents} parents")
    obj_bits = _bits_for(obj_max - obj_min + 1)
    if obj_bits + _bits_for(num_parents) > 63:
        raise ValueError(f"the (parent, obj) key needs {obj_bits + _bits_for(num_parents)} bits: "
                         f"objects span [{obj_min}, {obj_max}], at most 63 fit")
    return int(num_parents), obj_bits


def _merge_finish(pairs, parents, bad_parent, bad_pair, num_parents):
    if bad_pair:
        raise ValueError(f"merge_instances: {bad_pair} pair(s) that no cluster claims: pointers "
                         f"are not a monotone 0 .. num_pairs sequence")
    if bad_parent:                                                  # (excluded by the extents)
        raise AssertionError(f"Expected contiguous indices in [0, max]: {bad_parent} pair(s) "
                             f"point outside")
    if parents != num_parents:                                      # sparse.py:28
        raise AssertionError(f"Indices must be dense: {num_parents - parents} of {num_parents} "
                             f"parents hold no pair")


def _merge_torch(data, idx, num_parents):
    obj = data.obj
    num_parents, obj_bits = _merge_layout(int(obj.min()), int(obj.max()), int(idx.min()),
                                          int(idx.max()), num_parents)
    ptr, p = data.pointers, data.num_items
    j = torch.arange(p)
    cl = (torch.searchsorted(ptr, j, right=True) - 1).clamp(0, data.num_groups - 1)
    bad_pair = int((~((ptr[cl] <= j) & (j < ptr[cl + 1]))).sum())
    par = idx[cl]
    key = (par << obj_bits) | (obj - obj.min())
    inv, perm = _consecutive(key)
    count = torch.zeros(perm.numel(), dtype=torch.int64).index_add_(0, inv, data.count)
    sizes = torch.bincount(par[perm], minlength=num_parents)
    _merge_finish(perm.numel(), int((sizes > 0).sum()), 0, bad_pair, num_parents)
    out = InstanceData(torch.cat([sizes.new_zeros(1), sizes.cumsum(0)]), obj[perm], count,
                       data.y[perm])
    out._obj_extent = (int(obj.min()), int(obj.max()))
    return out


def merge_instances(instance_data, idx, num_parents=None):
    """``instance_data.merge(idx)``: the clusters merged into the parents ``idx`` (int ``[G]``,
    every value of ``[0, num_parents)`` present; ``num_parents`` defaults to ``idx.max() + 1``).
    Pairs are re-keyed by ``(idx[cluster], obj)``, duplicates of a key become one pair with their
    counts summed, the result is sorted by ``(parent, obj)`` and ``y`` is that of the last pair
    holding the key.  Object ids are taken relative to their minimum, so sparse ids past 2^31
    cost no more than their spread.

    Raises ``AssertionError`` as the reference does (wrong shape of ``idx``, no pair, indices not
    contiguous in ``[0, max]``, a parent left without a pair) and ``ValueError`` for a key beyond
    63 bits or pointers that are no CSR.  Two host reads on the device (module docstring)."""
    idx = torch.as_tensor(idx, device=instance_data.device)
    _merge_checks(instance_data, idx, num_parents)
    d = instance_data
    idx = idx.detach().long().contiguous()
    if not d.pointers.is_cuda:
        return _merge_torch(d, idx, num_parents)
    dev, p, g = d.device, d.num_items, d.num_groups
    L, stream = _lib.lib, _lib.stream_ptr(dev)
    extents = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = L.spt_instance_extents_i64(_lib.ptr(d.obj), p, _lib.ptr(idx), g, _lib.ptr(extents),
                                        stream)
    _lib.check(st, "spt_instance_extents_i64")
    obj_min, obj_max, idx_min, idx_max = extents.tolist()           # host read 1: the extents
    num_parents, obj_bits = _merge_layout(obj_min, obj_max, idx_min, idx_max, num_parents)
    key_bits = obj_bits + _bits_for(num_parents)
    pointers = torch.empty(num_parents + 1, dtype=torch.int64, device=dev)
    obj = torch.empty(p, dtype=torch.int64, device=dev)
    count = torch.empty(p, dtype=torch.int64, device=dev)
    y = torch.empty(p, dtype=torch.int64, device=dev)
    record = torch.zeros(4, dtype=torch.int64, device=dev)
    nbytes = L.spt_merge_instances_workspace_bytes(p, key_bits)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_merge_instances_i64(
            _lib.ptr(d.pointers), _lib.ptr(d.obj), _lib.ptr(d.count), _lib.ptr(d.y), _lib.ptr(idx),
            g, p, num_parents, obj_min, obj_bits, _lib.ptr(pointers), _lib.ptr(obj),
            _lib.ptr(count), _lib.ptr(y), _lib.ptr(record), _lib.ptr(ws), nbytes, stream)
    _lib.check(st, "spt_merge_instances_i64")
    pairs, parents, bad_parent, bad_pair = record.tolist()          # host read 2: the record
    _merge_finish(pairs, parents, bad_parent, bad_pair, num_parents)
    out = InstanceData(pointers, obj[:pairs], count[:pairs], y[:pairs])
    out._obj_extent = (obj_min, obj_max)
    return out


# ------------------------------------------------------------------------------------------------
def _obj_key_range(d):
    """(obj_lo, obj_bits) of the object sort: from the extents ``merge_instances`` left on its
    result, else the whole non-negative int64 range - no host read either way."""
    extent = getattr(d, "_obj_extent", None)
    if extent is None:
        return 0, 63
    return extent[0], _bits_for(extent[1] - extent[0] + 1)


def _stats_torch(d, c, status):
    p, g = d.num_items, d.num_groups
    ptr, count, y, obj = d.pointers, d.count, d.y, d.obj
    j = torch.arange(p)
    cl = (torch.searchsorted(ptr, j, right=True) - 1).clamp(0, g - 1)
    bad = int((~((ptr[cl] <= j) & (j < ptr[cl + 1]))).sum()) + int((ptr[1:] < ptr[:-1]).sum()) \
        + int(bool(ptr[0] != 0) or bool(ptr[-1] != p))
    obj_lo, obj_bits = _obj_key_range(d)
    status[0] += bad
    status[1] += int(((obj < obj_lo) | (((obj - obj_lo) >> obj_bits) != 0)).sum())
    y_void = (y < 0) | (y >= c)
    cl_size = torch.zeros(g, dtype=torch.int64).index_add_(0, cl, count)
    cl_void = torch.zeros(g, dtype=torch.int64).index_add_(0, cl, count * y_void)
    is_cluster_void = (cl_void / cl_size.float()) > 0.5
    uniq, inv = torch.unique(obj, return_inverse=True)
    b_sum = torch.zeros(uniq.numel(), dtype=torch.int64).index_add_(0, inv, count)[inv]
    cropped = torch.zeros(uniq.numel(), dtype=torch.int64).index_add_(
        0, inv, count * is_cluster_void[cl])[inv]
    a_size = cl_size[cl]
    b_size = b_sum if d.pair_cropped_count is None else b_sum + d.pair_cropped_count
    iou = count / (a_size + b_size - count)
    pair_void = y_void | is_cluster_void[cl]
    kept_iou = count / ((cl_size - cl_void)[cl] + b_sum - count)
    kept_iou = torch.where(pair_void, torch.zeros_like(kept_iou), kept_iou)
    keep = ~pair_void
    last = torch.full((uniq.numel(),), -1, dtype=torch.int64)
    last.scatter_reduce_(0, inv[keep], j[keep], "amax", include_self=True)
    gt_head = torch.zeros(p, dtype=torch.bool)
    gt_head[last[last >= 0]] = True
    return SimpleNamespace(a_size=a_size, b_size=b_size, iou=iou, is_cluster_void=is_cluster_void,
                           is_pair_void=pair_void, pair_cropped_count=cropped, kept_iou=kept_iou,
                           gt_head=gt_head, status=status)


def pair_stats(instance_data, num_classes, status=None):
    """Per pair of ``instance_data`` and for ``num_classes`` valid labels (anything else is void):

    ``a_size, b_size, iou``  ``iou_and_size()``: points of the pair's cluster, of its object
                             (plus ``pair_cropped_count`` when the data carries one), and
                             ``count / (a_size + b_size - count)`` as torch divides int64 tensors;
    ``is_cluster_void, is_pair_void, pair_cropped_count``  ``search_void(num_classes)``;
    ``kept_iou``             the pair's IoU in ``remove_void(num_classes)[0].iou_and_size()``
                             (0 for a void pair): nothing is compacted;
    ``gt_head``              True on the last non-void pair of each object.

    Returns a namespace of these and ``status`` (int32 ``[4]``, added to; a fresh one when not
    given; ``raise_status`` names its words).  No host read."""
    d, c = instance_data, int(num_classes)
    if c < 1:
        raise ValueError("num_classes must be positive")
    if d.num_items == 0:
        raise AssertionError("At least one group index is required.")
    _check_data(d)
    dev = d.device
    if status is None:
        status = torch.zeros(STATUS_WORDS, dtype=torch.int32, device=dev)
    if not d.pointers.is_cuda:
        return _stats_torch(d, c, status)
    p, g = d.num_items, d.num_groups
    obj_lo, obj_bits = _obj_key_range(d)
    cropped_in = d.pair_cropped_count
    if cropped_in is not None:
        cropped_in = cropped_in.long().contiguous()
    a_size = torch.empty(p, dtype=torch.int64, device=dev)
    b_size = torch.empty(p, dtype=torch.int64, device=dev)
    cropped = torch.empty(p, dtype=torch.int64, device=dev)
    iou = torch.empty(p, dtype=torch.float32, device=dev)
    kept_iou = torch.empty(p, dtype=torch.float32, device=dev)
    cluster_void = torch.empty(g, dtype=torch.bool, device=dev)
    pair_void = torch.empty(p, dtype=torch.bool, device=dev)
    gt_head = torch.empty(p, dtype=torch.bool, device=dev)
    L = _lib.lib
    nbytes = L.spt_pair_stats_workspace_bytes(p, g, obj_bits)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_pair_stats_i64(
            _lib.ptr(d.pointers), _lib.ptr(d.obj), _lib.ptr(d.count), _lib.ptr(d.y),
            _lib.ptr(cropped_in), g, p, c, obj_lo, obj_bits, _lib.ptr(a_size), _lib.ptr(b_size),
            _lib.ptr(iou), _lib.ptr(cluster_void), _lib.ptr(pair_void), _lib.ptr(cropped),
            _lib.ptr(kept_iou), _lib.ptr(gt_head), _lib.ptr(status), _lib.ptr(ws), nbytes,
            _lib.stream_ptr(dev))
    _lib.check(st, "spt_pair_stats_i64")
    return SimpleNamespace(a_size=a_size, b_size=b_size, iou=iou, is_cluster_void=cluster_void,
                           is_pair_void=pair_void, pair_cropped_count=cropped, kept_iou=kept_iou,
                           gt_head=gt_head, status=status)


# ------------------------------------------------------------------------------------------------
def new_state(num_classes, device=None):
    """The state of ``panoptic_counts_``: ``[5, C]`` 8-byte words - rows ``tp``, ``gt_count``,
    ``pred_count`` int64, rows ``iou_sum``, ``iou_mod_sum`` float64 (``state_views``)."""
    return torch.zeros(5, int(num_classes), dtype=torch.int64, device=device)


def state_views(state):
    """``(tp, gt_count, pred_count, iou_sum, iou_mod_sum)``: views of the state's rows, the
    last two as float64.  Five small tensors that sum across ranks."""
    f = state[3:].view(torch.float64)
    return state[0], state[1], state[2], f[0], f[1]


def _counts_torch(state, pred, d, c, stuff, s):
    keep = ~s.is_pair_void
    y = d.y
    cl = d.indices
    tp, gt, pc, iou_sum, iou_mod = state_views(state)
    gt += torch.bincount(y[s.gt_head & keep], minlength=c)
    p_valid = pred[~s.is_cluster_void]
    in_range = (p_valid >= 0) & (p_valid < c)
    pc += torch.bincount(p_valid[in_range], minlength=c)
    s.status[2] += int((~in_range).sum())
    l, q, ps = y[keep], s.kept_iou[keep], pred[cl[keep]]
    agree = ps == l
    ok = (q >= 0) & (q <= 1)
    s.status[3] += int((agree & ~ok).sum())
    is_tp = agree & ok & (q > 0.5)
    is_mod = agree & ok & ((q > 0.5) | stuff[l].bool())
    tp += torch.bincount(l[is_tp], minlength=c)
    dq = q.double() * 4294967296.0
    hi = dq.floor()
    lo = ((dq - hi) * 4294967296.0).floor().long()
    hi = hi.long()
    for mask, row in ((is_tp, iou_sum), (is_mod, iou_mod)):
        h = torch.zeros(c, dtype=torch.int64).index_add_(0, l[mask], hi[mask])
        w = torch.zeros(c, dtype=torch.int64).index_add_(0, l[mask], lo[mask])
        row += h.double() * 2.3283064365386963e-10 + w.double() * 5.421010862427522e-20
    return state


def panoptic_counts_(state, pred_semantic, instance_data, num_classes, stuff_mask, stats=None):
    """Add one batch into ``state`` (``new_state``), as ``PanopticQuality3D.compute`` counts it:
    a pair is removed if its object is void or its cluster is more than half void; ``gt_count``
    takes one per object that keeps a pair, by its ``y``; ``pred_count`` one per non-void cluster,
    by ``pred_semantic`` (int64 ``[G]``); a pair whose classes agree and whose IoU after void
    removal is ``> 0.5`` (strictly) adds to ``tp`` and ``iou_sum``, that or a stuff class
    (``stuff_mask``: bool / uint8 ``[C]``) to ``iou_mod_sum``.

    The two float sums are deterministic: every IoU is added as a 64 + 64-bit fixed-point
    integer, and one float64 add per class and call brings the call's sum into the state.
    ``stats``: the ``pair_stats`` of the same data, computed here when not given; faults are
    counted in ``stats.status``.  No host read.  Returns ``stats``."""
    d, c = instance_data, int(num_classes)
    if stats is None:
        stats = pair_stats(d, c)
    dev = d.device
    if state.dtype != torch.int64 or tuple(state.shape) != (5, c) or not state.is_contiguous() \
            or state.device != dev:
        raise ValueError(f"state must be a contiguous int64 [5, {c}] tensor on {dev}")
    if not isinstance(pred_semantic, torch.Tensor) or pred_semantic.dtype != torch.long:
        raise ValueError("Expected argument `prediction_semantic` to be a Tensor of dtype=long")
    if pred_semantic.dim() != 1 or pred_semantic.numel() != d.num_groups:
        raise ValueError("Expected argument `prediction_semantic` to hold one label per cluster "
                         "of `instance_data`")
    if pred_semantic.device != dev or stuff_mask.device != dev:
        raise ValueError(f"prediction_semantic and stuff_mask must live on {dev}")
    if stuff_mask.numel() != c or stuff_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"stuff_mask must be a bool or uint8 [{c}] tensor")
    pred = pred_semantic.detach().contiguous()
    stuff = stuff_mask.contiguous()
    if not state.is_cuda:
        _counts_torch(state, pred, d, c, stuff, stats)
        return stats
    if c > MAX_CLASSES:
        raise ValueError(f"the device tables hold at most {MAX_CLASSES} classes, got {c}")
    L = _lib.lib
    nbytes = L.spt_panoptic_counts_workspace_bytes(c)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_panoptic_counts_i64(
            _lib.ptr(state), _lib.ptr(pred), _lib.ptr(d.pointers), _lib.ptr(d.y),
            _lib.ptr(stats.is_pair_void), _lib.ptr(stats.kept_iou), _lib.ptr(stats.gt_head),
            _lib.ptr(stats.is_cluster_void), d.num_groups, d.num_items, c, _lib.ptr(stuff),
            _lib.ptr(stats.status), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    _lib.check(st, "spt_panoptic_counts_i64")
    return stats


# ------------------------------------------------------------------------------------------------
def semantic_score(logits):
    """``logits.softmax(dim=1).max(dim=1).values`` evaluated in float64 and rounded to f32 once:
    within half an f32 ulp of the score of the given logits on every device."""
    return logits.double().softmax(dim=1).max(dim=1).values.float()


def weighted_group_mean(x, idx, w, num_groups, check=True):
    """``scatter_mean_weighted(x, idx, w, dim_size=num_groups)``: f32 ``[num_groups, C]`` (``x``
    ``[N]`` is taken as ``[N, 1]``), ``w`` cast to f32, the products ``x * w`` rounded before they
    are added, each group summed from 0 in ascending row order, a zero weight sum replaced by 1,
    one division.  Groups of up to ``SEQUENTIAL_ROWS`` rows equal the reference's CPU result bit
    for bit; longer ones are summed on the device in float64 (exact products, 64 strided partial
    sums joined by a fixed tree) and rounded to f32 once.  A group without a
    row gives 0.  The sign of the weights is not checked (the reference's assertion is a host
    read).  An ``idx`` outside ``[0, num_groups)`` is left out and reported - by
    ``ValueError`` under ``check=True`` (one host read), not at all under ``check=False``."""
    if w.dim() != 1 or idx.dim() != 1:
        raise AssertionError("w and idx should be 1D Tensors")
    if not (x.shape[0] == w.shape[0] == idx.shape[0]):
        raise AssertionError("Only supports weighted mean along the first dimension")
    if idx.is_floating_point():
        raise ValueError("idx must be an integer tensor")
    if x.dim() > 2 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [N] or [N, C] tensor")
    g = int(num_groups)
    n = x.shape[0]
    if g < 1 or g > MAX_ITEMS or n > MAX_ITEMS:
        raise ValueError(f"num_groups and the row count must lie in 1 .. {MAX_ITEMS}")
    x = x.detach().view(n, -1).contiguous()
    cols = x.shape[1]
    if cols < 1 or cols > 4096:
        raise ValueError("x must hold 1 .. 4096 columns")
    w = w.detach().float().contiguous()
    idx = idx.detach().long().contiguous()
    dev = x.device
    if w.device != dev or idx.device != dev:
        raise ValueError(f"idx and w must live on {dev}, with x")
    if not x.is_cuda:
        ok = (idx >= 0) & (idx < g)
        wx = torch.cat((w.view(-1, 1), x * w.view(-1, 1)), dim=1)
        seg = torch.zeros(g, cols + 1).index_add_(0, idx[ok], wx[ok])
        w_seg = seg[:, 0]
        w_seg[w_seg == 0] = 1
        out = seg[:, 1:] / w_seg.view(-1, 1)
        if check and not bool(ok.all()):
            raise ValueError(f"weighted_group_mean: {int((~ok).sum())} index entries outside "
                             f"[0, {g})")
        return out
    out = torch.empty(g, cols, dtype=torch.float32, device=dev)
    if n == 0:
        return out.zero_()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    L = _lib.lib
    nbytes = L.spt_weighted_group_mean_workspace_bytes(n, g)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_weighted_group_mean_f32(_lib.ptr(x), n, cols, _lib.ptr(idx), _lib.ptr(w), g,
                                           _lib.ptr(out), _lib.ptr(status), _lib.ptr(ws), nbytes,
                                           _lib.stream_ptr(dev))
    _lib.check(st, "spt_weighted_group_mean_f32")
    if check:
        bad = status.tolist()[0]                                    # the host read
        if bad:
            raise ValueError(f"weighted_group_mean: {bad} index entries outside [0, {g})")
    return out


# ------------------------------------------------------------------------------------------------
_MAJOR_FAULTS = ("{n} cluster(s) without a pair (the reference indexes out of range there)",
                 "{n} fault(s) of pointers (not a monotone 0 .. num_pairs sequence)")
_MAJOR_PENDING = []       # deferred verdicts of major_objects(check=True): (event | None, status)


def _raise_major(words):
    msgs = [_MAJOR_FAULTS[k].format(n=n) for k, n in enumerate(words) if n]
    if msgs:
        raise ValueError("major_objects: " + "; ".join(msgs))


def verify_major(block=False):
    """Read the statuses of the ``major_objects(check=True)`` calls that have COMPLETED
    (``block``: wait for all of them, those recorded inside a captured graph included) and raise
    ``ValueError`` for the first that counted a fault.  Never waits on the device unless asked."""
    keep, failed = [], None
    for ev, status in _MAJOR_PENDING:
        if ev is None and not block:
            keep.append((ev, status))
            continue
        if ev is not None:
            if block:
                ev.synchronize()
            if not ev.query():
                keep.append((ev, status))
                continue
        words = status.tolist()
        if any(words) and failed is None:
            failed = words
    _MAJOR_PENDING[:] = keep
    if failed is not None:
        _raise_major(failed)


def _first_argmax(values, cl, g):
    """Per cluster the lowest pair index holding the cluster's largest value (``g`` where the
    cluster is empty), and that value."""
    p = values.numel()
    best = torch.full((g,), torch.iinfo(torch.int64).min, dtype=torch.int64)
    best.scatter_reduce_(0, cl, values, "amax", include_self=True)
    j = torch.arange(p)
    hit = values == best[cl]
    arg = torch.full((g,), p, dtype=torch.int64)
    arg.scatter_reduce_(0, cl[hit], j[hit], "amin", include_self=True)
    return arg, best


def _major_torch(d, c):
    g, p = d.num_groups, d.num_items
    ptr = d.pointers
    sizes = ptr[1:] - ptr[:-1]
    bad_ptr = int(bool(ptr[0] != 0) or bool(ptr[-1] != p)) + int((sizes < 0).sum())
    if bad_ptr:
        _raise_major((0, bad_ptr))
    cl = torch.arange(g).repeat_interleave(sizes)
    void = (d.y < 0) | (d.y >= c)
    arg, count = _first_argmax(d.count, cl, g)
    arg_nv, count_nv = _first_argmax(d.count * ~void, cl, g)
    empty = arg >= p
    a, a_nv = arg.clamp(max=p - 1), arg_nv.clamp(max=p - 1)
    obj, y = d.obj[a], d.y[a]
    major_void = ((y < 0) | (y >= c)) & ~empty
    total = torch.zeros(g, dtype=torch.int64).index_add_(0, cl, d.count)
    above = (count / total) > 0.5                                   # int64 / int64: f32 division
    flag = (major_void & ~above).any()
    take = major_void & flag
    obj = torch.where(take, d.obj[a_nv], obj)
    count = torch.where(take, count_nv, count)
    y = torch.where(take, d.y[a_nv], y)
    fill = torch.tensor(-1)
    obj, y = torch.where(empty, fill, obj), torch.where(empty, fill, y)
    count = torch.where(empty, torch.tensor(0), count)
    return obj, count, y, int(empty.sum())


def major_objects(instance_data, num_classes, check=True, status=None):
    """``instance_data.major(num_classes)``: ``(obj, count, y)``, each int64 ``[num_clusters]`` -
    per cluster the pair of the largest ``count`` (ties: the first pair of the cluster).  A pair
    is void with ``y < 0`` or ``y >= num_classes``.  As the reference BEHAVES: if any cluster
    whose largest pair is void holds it with ``count / total <= 0.5`` (int64 operands, divided as
    f32), every cluster whose largest pair is void - those above one half included - takes the
    pair of the largest ``count * ~void`` instead (an all-void cluster: its first pair, count 0);
    otherwise none does.  On the device the decision is a flag between two kernels: no host read.

    A cluster without a pair makes the reference index out of range; here it gets ``obj = -1,
    count = 0, y = -1`` and is counted in ``status`` (int32 ``[2]``, added to: empty clusters,
    faults of ``pointers``; a fresh one when not given).  ``check=True`` defers the verdict as
    the CSR checks do: the status is read - without waiting - by a later ``major_objects`` call
    or by ``verify_major(block=True)``, which raise ``ValueError``; CPU tensors raise at once.
    ``check=False`` reports nothing; every access stays in bounds either way."""
    d, c = instance_data, int(num_classes)
    if c < 1:
        raise ValueError("num_classes must be positive")
    if d.num_items == 0:
        raise AssertionError("At least one group index is required.")
    _check_data(d)
    dev = d.device
    if not d.pointers.is_cuda:
        obj, count, y, empty = _major_torch(d, c)
        if status is not None:
            status[0] += empty
        if check and empty:
            _raise_major((empty, 0))
        return obj, count, y
    capturing = torch.cuda.is_current_stream_capturing()
    if _MAJOR_PENDING and not capturing:
        verify_major()
    g, p = d.num_groups, d.num_items
    if status is None:
        status = torch.zeros(2, dtype=torch.int32, device=dev)
    obj = torch.empty(g, dtype=torch.int64, device=dev)
    count = torch.empty(g, dtype=torch.int64, device=dev)
    y = torch.empty(g, dtype=torch.int64, device=dev)
    L = _lib.lib
    nbytes = L.spt_instance_major_workspace_bytes(g)
    ws = _workspace(nbytes, dev)
    with torch.cuda.device(dev):
        st = L.spt_instance_major_i64(_lib.ptr(d.pointers), _lib.ptr(d.obj), _lib.ptr(d.count),
                                      _lib.ptr(d.y), g, p, c, _lib.ptr(obj), _lib.ptr(count),
                                      _lib.ptr(y), _lib.ptr(status), _lib.ptr(ws), nbytes,
                                      _lib.stream_ptr(dev))
    _lib.check(st, "spt_instance_major_i64")
    if check and capturing:
        _MAJOR_PENDING.append((None, status))                       # read on request only
    elif check:
        host = torch.empty(2, dtype=torch.int32).pin_memory()
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        _MAJOR_PENDING.append((ev, host))
    return obj, count, y
