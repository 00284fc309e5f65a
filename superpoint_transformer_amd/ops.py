"""Functional, differentiable front-ends of the HIP segment kernels.

Every function here launches a kernel of libspt_hip.so on torch's current
stream; there is no eager-PyTorch path.  The one exception is the criterion
(``histogram_loss``, ``cross_entropy(weight=...)``, ``histogram_confusion_matrix``):
CPU tensors and heads wider than 32 classes take a torch composition of the
same closed forms, so that criterion and metric modules also run off the device.
"""
import contextlib
import ctypes
import os

import torch

from . import _lib
from . import precision as _precision
from .csr import EdgeCSR, SegmentCSR, csr_of, edge_csr_of

_OPS = {"sum": 0, "add": 0, "mean": 1, "min": 2, "max": 3}

# Optional per-kernel HIP-event timers (bench.py's roofline leg): name -> list
# of (start, end) events recorded on the stream the kernel is launched on.
_TIMERS = {}
_TIMER_PREFIXES = []
_TIMER_CAP = 8192            # event pairs kept per timer (timers are opt-in measurement aids)


def enable_timer(name, prefix=False):
    """Record a HIP event pair (torch's current stream = the launch stream) around every call site
    named ``name`` (``prefix=True``: every site whose name starts with it, pooled under it)."""
    _TIMERS[name] = []
    if prefix and name not in _TIMER_PREFIXES:
        _TIMER_PREFIXES.append(name)


def timer_count(name):
    return len(_TIMERS.get(name) or [])


def timer_mean_ms(name):
    pairs = _TIMERS.get(name) or []
    if not pairs:
        return None
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / len(pairs)


def reset_timers():
    for k in _TIMERS:
        _TIMERS[k] = []


_TIMERS_PAUSED = False


def pause_timers(on=True):
    """Stop / resume recording event pairs (a stream capture cannot hold timing events; a second
    workload timed next to the first must not pool into its timers).  Returns the old setting."""
    global _TIMERS_PAUSED
    old, _TIMERS_PAUSED = _TIMERS_PAUSED, bool(on)
    return old


_CONST = {}
_KEEP = []           # the lists of the active keep_handed_out() blocks, innermost last


@contextlib.contextmanager
def keep_handed_out(into):
    """Inside the block every tensor that ``_const_tensor`` or ``_workspace`` hands out is also
    appended to the list ``into`` (once).  Kernels get these tensors as raw addresses, so a captured
    graph reads them without holding a reference, while ``_CONST`` is cleared past 512 keys and a
    stream's scratch is replaced when a larger one is asked for: whoever captures keeps ``into``
    for as long as the graph lives (``hotpath.SPTTrainStep.capture``)."""
    _KEEP.append(into)
    try:
        yield into
    finally:
        _KEEP.pop()


def _handed_out(t):
    for kept in _KEEP:
        if not any(t is u for u in kept):
            kept.append(t)
    return t


def _const_tensor(vals, dtype, dev):
    """Small host-known table as a device tensor, uploaded ONCE per (values, dtype, device): a
    fresh ``torch.tensor(list, device=...)`` is a pageable host-to-device copy - a stall in an
    eager step and not capturable into a graph."""
    key = (tuple(vals), dtype, dev.index)
    t = _CONST.get(key)
    if t is None:
        if len(_CONST) > 512:
            _CONST.clear()
        t = _CONST[key] = torch.tensor(list(vals), dtype=dtype, device=dev)
    return _handed_out(t)


class _timed:
    def __init__(self, name):
        self.rec = None if _TIMERS_PAUSED else _TIMERS.get(name)
        if _TIMERS_PAUSED:
            return
        if self.rec is None and _TIMER_PREFIXES:
            for p in _TIMER_PREFIXES:
                if name.startswith(p):
                    self.rec = _TIMERS[p]
                    break

    def __enter__(self):
        if self.rec is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            if len(self.rec) >= _TIMER_CAP:      # a loop longer than a benchmark: keep the newest
                del self.rec[:_TIMER_CAP // 2]
            self.rec.append((self.a, b))


_dense = _lib.dense          # the one place a tensor's layout is turned into the kernels' contract


def _as_rows(x):
    """[n, ...] -> contiguous, 16B-aligned f32 [n, c] plus the trailing shape."""
    tail = x.shape[1:]
    return _dense(x.reshape(x.shape[0], -1), torch.float32), tail


def _seg_reduce_fwd(x2, csr, op, want_arg):
    n, c = x2.shape
    out = torch.empty((csr.num_seg, c), dtype=torch.float32, device=x2.device)
    arg = None
    if want_arg and op in (2, 3):
        arg = torch.empty((csr.num_seg, c), dtype=torch.int32, device=x2.device)
    with torch.cuda.device(x2.device), _timed(f"segcsr_reduce_fwd:{op}:{n}x{c}"):
        st = _lib.lib.spt_segcsr_reduce_f32(
            op, _lib.ptr(x2), _lib.ptr(csr.perm), _lib.ptr(csr.rowptr), n,
            csr.num_seg, c, _lib.ptr(out), _lib.ptr(arg), _lib.stream_ptr(x2.device))
    _lib.check(st, "spt_segcsr_reduce_f32")
    return out, arg


def _seg_reduce_bwd(gout, arg, csr, op, n):
    c = gout.shape[1]
    gx = torch.empty((n, c), dtype=torch.float32, device=gout.device)
    with torch.cuda.device(gout.device), _timed(f"segcsr_reduce_bwd:{op}:{n}x{c}"):
        st = _lib.lib.spt_segcsr_reduce_bwd_f32(
            op, _lib.ptr(gout), _lib.ptr(arg), _lib.ptr(csr.idx),
            _lib.ptr(csr.perm), _lib.ptr(csr.rowptr), n, csr.num_seg, c, _lib.ptr(gx),
            _lib.stream_ptr(gout.device))
    _lib.check(st, "spt_segcsr_reduce_bwd_f32")
    return gx


def _gather_fwd(x2, idx):
    n = idx.numel()
    c = x2.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=x2.device)
    with torch.cuda.device(x2.device):
        st = _lib.lib.spt_gather_rows_f32(
            _lib.ptr(x2), _lib.ptr(idx), n, x2.shape[0], c, _lib.ptr(out),
            _lib.stream_ptr(x2.device))
    _lib.check(st, "spt_gather_rows_f32")
    return out


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, csr, op, want_arg):
        _lib.require_cuda(x)
        x2, tail = _as_rows(x)
        if x2.shape[0] != csr.n:
            raise ValueError(
                f"src has {x2.shape[0]} rows but the index has {csr.n}")
        need_arg = op in (2, 3) and (want_arg or x.requires_grad)
        out, arg = _seg_reduce_fwd(x2, csr, op, need_arg)
        ctx.csr, ctx.op, ctx.n, ctx.tail, ctx.in_dtype = csr, op, x2.shape[0], tail, x.dtype
        ctx.save_for_backward(arg)
        out = out.reshape((csr.num_seg,) + tuple(tail)).to(x.dtype)
        if arg is not None:
            arg_out = arg.reshape((csr.num_seg,) + tuple(tail))
            ctx.mark_non_differentiable(arg_out)
            return out, arg_out
        return out, None

    @staticmethod
    def backward(ctx, gout, _garg):
        (arg,) = ctx.saved_tensors
        g2, _ = _as_rows(gout)
        gx = _seg_reduce_bwd(g2, arg, ctx.csr, ctx.op, ctx.n)
        return gx.reshape((ctx.n,) + tuple(ctx.tail)).to(ctx.in_dtype), None, None, None


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, csr_holder):
        _lib.require_cuda(x, idx)
        x2, tail = _as_rows(x)
        idx = _dense(idx, torch.int64, 8)
        ctx.idx, ctx.holder = idx, csr_holder
        ctx.num_src, ctx.tail, ctx.in_dtype = x2.shape[0], tail, x.dtype
        out = _gather_fwd(x2, idx)
        return out.reshape((idx.numel(),) + tuple(tail)).to(x.dtype)

    @staticmethod
    def backward(ctx, gout):
        g2, _ = _as_rows(gout)
        # backward of a gather is a segment sum over the CSR view of idx
        csr = csr_of(ctx.holder if ctx.holder is not None else ctx.idx, ctx.num_src)
        gx, _ = _seg_reduce_fwd(g2, csr, 0, False)
        return gx.reshape((ctx.num_src,) + tuple(ctx.tail)).to(ctx.in_dtype), None, None


def segment_reduce(x, index, num_seg=None, reduce="sum", return_arg=False):
    """out[s] = reduce_{i: index[i]==s} x[i] along dim 0 (empty -> 0).

    ``index`` is an int64 [n] tensor or a prebuilt :class:`SegmentCSR`.
    For min/max and ``return_arg=True`` also returns the int32 arg rows
    (``n`` for empty segments).
    """
    op = _OPS[reduce]
    csr = csr_of(index, num_seg)
    out, arg = _SegmentReduce.apply(x, csr, op, return_arg)
    if return_arg:
        return out, arg
    return out


def gather_rows(x, idx):
    """out[i] = x[idx[i]]  (IndexUnpool forward; backward = segment sum)."""
    return _GatherRows.apply(x, idx, idx)


class _EdgeAffinityFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, edge_index):
        _lib.require_cuda(x, edge_index)
        xc = _dense(x.detach(), torch.float32)
        ei = _dense(edge_index, torch.int64, 8)
        n, c = xc.shape
        e = ei.shape[1]
        out = torch.empty((e, 2 * c), dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            st = _lib.lib.spt_edge_affinity_features_f32(
                _lib.ptr(xc), n, c, _lib.ptr(ei[0]), _lib.ptr(ei[1]), e, _lib.ptr(out),
                _lib.stream_ptr(xc.device))
        _lib.check(st, "spt_edge_affinity_features_f32")
        ctx.save_for_backward(xc, ei)
        ctx.in_dtype = x.dtype
        return out.to(x.dtype)

    @staticmethod
    def backward(ctx, gout):
        xc, ei = ctx.saved_tensors
        n, c = xc.shape
        e = ei.shape[1]
        g = _dense(gout, torch.float32)
        gend = torch.empty((2 * e, c), dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            st = _lib.lib.spt_edge_affinity_features_bwd_f32(
                _lib.ptr(xc), _lib.ptr(g), n, c, _lib.ptr(ei[0]), _lib.ptr(ei[1]), e,
                _lib.ptr(gend), _lib.stream_ptr(xc.device))
        _lib.check(st, "spt_edge_affinity_features_bwd_f32")
        # per-node sums over both endpoint lists: one CSR segment reduce (memoised on the
        # edge_index tensor's flattened view for the lifetime of the batch)
        gx, _ = _seg_reduce_fwd(gend, csr_of(ei.reshape(-1), n), 0, False)
        return gx.to(ctx.in_dtype), None


def edge_affinity_features(x, edge_index):
    """``cat(|x[a] - x[b]|, (x[a] + x[b]) / 2)`` for the edges ``(a, b) = edge_index``
    (src/models/panoptic.py:477-480), one fused pass each way."""
    return _EdgeAffinityFeatures.apply(x, edge_index)


def segment_sum_i64(x, index, num_seg=None):
    """Bit-exact int64 segment sum (NAG.get_sub_size chain)."""
    _lib.require_cuda(x)
    csr = csr_of(index, num_seg)
    tail = x.shape[1:]
    x2 = _dense(x.reshape(x.shape[0], -1), torch.int64, 8)
    c = x2.shape[1]
    out = torch.empty((csr.num_seg, c), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        st = _lib.lib.spt_segcsr_sum_i64(
            _lib.ptr(x2), _lib.ptr(csr.perm), _lib.ptr(csr.rowptr), x2.shape[0],
            csr.num_seg, c, _lib.ptr(out), _lib.stream_ptr(x.device))
    _lib.check(st, "spt_segcsr_sum_i64")
    return out.reshape((csr.num_seg,) + tuple(tail))


# ---------------------------------------------------------------------------
# UnitSphereNorm (src/nn/norm.py:67-138)
# ---------------------------------------------------------------------------
def _usn_args(pos, idx, w, num_super):
    _lib.require_cuda(pos)
    pos = _dense(pos.detach(), torch.float32)
    n = pos.shape[0]
    dev = pos.device
    if idx is None:
        num_seg = 1
        perm = None
        rowptr = _const_tensor([0, n], torch.int32, dev)
        idx_t = None
    else:
        csr = csr_of(idx, num_super)
        num_seg, perm, rowptr, idx_t = csr.num_seg, csr.perm, csr.rowptr, csr.idx
    wf = wi = None
    if w is not None:
        w = w.detach()
        if w.is_floating_point():
            wf = _dense(w, torch.float32)
        else:
            wi = _dense(w, torch.int64, 8)
    return pos, n, dev, num_seg, perm, rowptr, idx_t, wf, wi


def unit_sphere_norm(pos, idx, w=None, num_super=None):
    """Returns (pos_normalised [n,3], diameter [num_super,1]) like
    UnitSphereNorm.forward with log_diameter=False.  ``idx=None`` normalises
    all rows together (norm.py:86-110).  No gradient: positions are data."""
    pos, n, dev, num_seg, perm, rowptr, idx_t, wf, wi = _usn_args(pos, idx, w, num_super)
    out = torch.empty_like(pos)
    diam = torch.empty(num_seg, dtype=torch.float32, device=dev)
    center = torch.empty((num_seg, 3), dtype=torch.float32, device=dev)
    nb = _lib.lib.spt_unit_sphere_workspace_bytes(n, num_seg)
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_unit_sphere_norm_ws_f32(
            _lib.ptr(pos), _lib.ptr(idx_t), _lib.ptr(perm), _lib.ptr(rowptr),
            _lib.ptr(wf), _lib.ptr(wi), n, num_seg, _lib.ptr(out), _lib.ptr(diam),
            _lib.ptr(center), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(st, "spt_unit_sphere_norm_ws_f32")
    return out, diam.view(-1, 1)


class _UnitSphereAssemble(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, idx, w, num_super):
        pos, n, dev, num_seg, perm, rowptr, idx_t, wf, wi = _usn_args(pos, idx, w, num_super)
        x2 = _f32c(x.detach())
        cx = x2.shape[1]
        out = torch.empty((n, 4 + cx), dtype=torch.float32, device=dev)
        diam = torch.empty(num_seg, dtype=torch.float32, device=dev)
        center = torch.empty((num_seg, 3), dtype=torch.float32, device=dev)
        nb = _lib.lib.spt_unit_sphere_workspace_bytes(n, num_seg)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_unit_sphere_assemble_ws_f32(
                _lib.ptr(pos), _lib.ptr(idx_t), _lib.ptr(perm), _lib.ptr(rowptr), _lib.ptr(wf),
                _lib.ptr(wi), n, num_seg, _lib.ptr(x2), cx, _lib.ptr(out), _lib.ptr(diam),
                _lib.ptr(center), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "spt_unit_sphere_assemble_ws_f32")
        diam = diam.view(-1, 1)
        ctx.mark_non_differentiable(diam)
        ctx.x_dtype = x.dtype
        return out, diam

    @staticmethod
    def backward(ctx, gout, _gdiam):
        return gout[:, 4:].to(ctx.x_dtype), None, None, None, None


def unit_sphere_assemble_ok(x, pos):
    """Whether ``unit_sphere_assemble`` applies: f32 CUDA features of a multiple of 4 columns."""
    return (torch.is_tensor(x) and torch.is_tensor(pos) and x.is_cuda and x.dim() == 2
            and x.dtype == torch.float32 and x.shape[1] >= 4 and x.shape[1] % 4 == 0
            and x.shape[0] == pos.shape[0])


def unit_sphere_assemble(x, pos, idx, w=None, num_super=None):
    """``(cat([diameter[idx], pos_normalised, x], 1), diameter)``: UnitSphereNorm and the three
    fusion concatenations of a stage's input (src/nn/stage.py:249-271 with ``use_pos`` and
    ``use_diameter_parent``) in one writing pass.  The gradient reaches ``x`` (a column slice)."""
    return _UnitSphereAssemble.apply(x, pos, idx, w, num_super)


# ---------------------------------------------------------------------------
# GraphNorm (+ fused LeakyReLU)
# ---------------------------------------------------------------------------
_WS = {}


def _workspace(nbytes, dev):
    """Grow-only scratch buffer per (device, stream).  Kernels that share it
    are ordered on the stream, so reuse across calls is safe."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _WS[key] = buf
    return _handed_out(buf)


class _GraphNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, batch, num_graphs, weight, bias, mean_scale, eps, slope):
        _lib.require_cuda(x)
        x2 = _dense(x, torch.float32)
        r, d = x2.shape
        dev = x2.device
        batch = _dense(batch, torch.int64, 8)
        w, b, a = (_dense(t.detach(), torch.float32) for t in (weight, bias, mean_scale))
        y = torch.empty_like(x2)
        mean = torch.empty((num_graphs, d), dtype=torch.float32, device=dev)
        rstd = torch.empty((num_graphs, d), dtype=torch.float32, device=dev)
        nb = _lib.lib.spt_graphnorm_workspace_bytes(r, d, num_graphs)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_graphnorm_fwd_f32(
                _lib.ptr(x2), _lib.ptr(batch), r, d, num_graphs, _lib.ptr(w),
                _lib.ptr(b), _lib.ptr(a), eps, slope, _lib.ptr(y), _lib.ptr(mean),
                _lib.ptr(rstd), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "spt_graphnorm_fwd_f32")
        ctx.save_for_backward(x2, batch, w, b, a, mean, rstd)
        ctx.meta = (num_graphs, slope, x.dtype)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        x2, batch, w, b, a, mean, rstd = ctx.saved_tensors
        num_graphs, slope, in_dtype = ctx.meta
        r, d = x2.shape
        dev = x2.device
        gy = _dense(gy, torch.float32)
        gx = torch.empty_like(x2)
        gw = torch.empty(d, dtype=torch.float32, device=dev)
        gb = torch.empty(d, dtype=torch.float32, device=dev)
        ga = torch.empty(d, dtype=torch.float32, device=dev)
        nb = _lib.lib.spt_graphnorm_workspace_bytes(r, d, num_graphs)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_graphnorm_bwd_f32(
                _lib.ptr(x2), _lib.ptr(gy), _lib.ptr(batch), r, d, num_graphs,
                _lib.ptr(w), _lib.ptr(b), _lib.ptr(a), _lib.ptr(mean), _lib.ptr(rstd),
                slope, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ga),
                _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "spt_graphnorm_bwd_f32")
        return gx.to(in_dtype), None, None, gw, gb, ga, None, None


_NGRAPHS_ATTR = "_spt_num_graphs"


def _num_graphs_of(batch):
    """``batch.max() + 1``, read back once per batch vector (memoised on the tensor object, keyed
    on its version like the CSR views; ``csr.forget`` drops it)."""
    key = (batch._version, batch.data_ptr(), batch.numel())
    memo = getattr(batch, _NGRAPHS_ATTR, None)
    if memo is not None and memo[0] == key:
        return memo[1]
    n = int(batch.max().item()) + 1 if batch.numel() else 1
    try:
        setattr(batch, _NGRAPHS_ATTR, (key, n))
    except Exception:
        pass
    return n


def graph_norm(x, batch, weight, bias, mean_scale, eps=1e-5, num_graphs=None,
               act_slope=1.0):
    """GraphNorm(x, batch) [+ LeakyReLU(act_slope) when act_slope != 1].
    ``num_graphs=None`` costs a host sync (``batch.max()+1``, once per batch vector) like
    PyG's GraphNorm; pass it to stay asynchronous."""
    if batch is None:
        num_graphs = 1
    elif num_graphs is None:
        num_graphs = _num_graphs_of(batch)
    return _GraphNorm.apply(x, batch, int(num_graphs), weight, bias, mean_scale,
                            float(eps), float(act_slope))


# ---------------------------------------------------------------------------
# Fused edge attention (src/nn/attention.py:202-315)
# ---------------------------------------------------------------------------
def _f32c(t):
    if t is None:
        return None
    return _dense(t.detach(), torch.float32)


_EA_SHARE = os.environ.get("SPT_EA_GRAD_SHARE", "1") != "0"


def share_edge_attr_grad(on=None):
    """Whether ``Stage.forward`` lets its blocks accumulate d edge_attr in one buffer (default on;
    ``SPT_EA_GRAD_SHARE=0`` in the environment turns it off).  Returns the previous setting."""
    global _EA_SHARE
    prev = _EA_SHARE
    if on is not None:
        _EA_SHARE = bool(on)
    return prev


class EdgeAttrGradShare:
    """One gradient buffer for the ``edge_attr`` of a stage: every transformer block of the
    stage reads the same ``edge_attr`` (src/nn/stage.py:137-141), so instead of each attention
    backward returning its own [E, F] tensor for autograd to sum, the blocks accumulate into one
    buffer (``spt_edge_attn_bwd_acc_f32``) and only the block that ran FIRST in the forward - the
    last one autograd reaches, every later block depends on its output - hands it to autograd.

    Valid for one forward pass over sequentially dependent blocks, which is what ``Stage.forward``
    creates it for; a backward that stops short of the first block (``autograd.grad`` on an
    intermediate block's inputs) would not see the edge_attr gradient - do not pass a share in
    that case.

    A backward that fails part-way, or one that re-enters a block before the first block has
    handed the buffer over (a retained graph walked again after a partial ``autograd.grad``),
    must not add onto what an earlier walk left behind: ``acquire`` starts a fresh buffer
    whenever the entering block has already been seen in the current walk, ``abort`` drops it."""

    __slots__ = ("tensor", "count", "buf", "seen")

    def __init__(self):
        self.tensor, self.count, self.buf, self.seen = None, 0, None, set()

    def acquire(self, rank, like):
        """(buffer, acc) for the block of forward order ``rank``: acc = 1 when a later block of
        THIS backward walk already started the sum."""
        if rank in self.seen:                # a second walk without a hand-over: stale state
            self.buf, self.seen = None, set()
        self.seen.add(rank)
        if self.buf is not None:
            return self.buf, 1
        self.buf = torch.empty_like(like)
        return self.buf, 0

    def release(self, rank):
        """The buffer if ``rank`` is the block that hands it to autograd (the first one of the
        forward), else None."""
        if rank != 0:
            return None
        buf, self.buf, self.seen = self.buf, None, set()
        return buf

    def abort(self):
        self.buf, self.seen = None, set()

    def enter(self, edge_attr):
        if self.tensor is None:
            self.tensor = edge_attr
        elif self.tensor is not edge_attr:
            raise ValueError("EdgeAttrGradShare: the blocks were given different edge_attr tensors")
        self.count += 1
        return self.count - 1


# operand bits and results of spt_edge_attn_bwd_route (include/spt_hip.h)
_ATTN_HAS_RPE, _ATTN_HAS_SRC, _ATTN_HAS_TILE_IDS, _ATTN_HAS_TARGET_VIEW = 1, 2, 4, 8
(ATTN_ROUTE_VALU, ATTN_ROUTE_PER_NODE, ATTN_ROUTE_PACKED, ATTN_ROUTE_EDGE_LANE_SOURCE,
 ATTN_ROUTE_EDGE_LANE_TARGET) = range(5)


def _attn_mode(mode=None):
    """The mode word of one ``edge_attention`` call, every field explicit: resolved ONCE, then
    handed to the forward, the tile records and (``ctx.mode``) the backward."""
    return int(_lib.lib.spt_attn_resolve_mode(_precision.attention_mode())) if mode is None else mode


def _attn_bwd_plan(ecsr, n, H, D, Dv, F, has_rpe, mode):
    """(route, workspace, src, tile_ids, tperm, trowptr) of an attention backward in the resolved
    ``mode``: the library names the route it takes when given everything (spt_edge_attn_bwd_route),
    that route's operands are prepared, and the route is asked for again with exactly these - a
    different answer would be a silent downgrade, and raises."""
    L, dev = _lib.lib, ecsr.tgt_sorted.device

    def route(operands, nbytes):
        r = L.spt_edge_attn_bwd_route(n, ecsr.e, H, D, Dv, F, operands, mode, nbytes)
        _lib.check(min(r, 0), "spt_edge_attn_bwd_route")
        return r

    operands = _ATTN_HAS_RPE if has_rpe else 0
    want = route(operands | _ATTN_HAS_SRC | _ATTN_HAS_TILE_IDS | _ATTN_HAS_TARGET_VIEW, 1 << 62)
    src = tids = tperm = trowptr = None
    if want in (ATTN_ROUTE_EDGE_LANE_SOURCE, ATTN_ROUTE_EDGE_LANE_TARGET):
        # the larger scratch is asked for only where it is used (the buffer is grow-only)
        nb = L.spt_edge_attn_bwd_ex_workspace_bytes(n, ecsr.e, H, D, Dv, F)
        src, tids = ecsr.src_sorted(), ecsr.tile_ids(mode)
        operands |= _ATTN_HAS_SRC | _ATTN_HAS_TILE_IDS
        if not ecsr.mirrored(mode):
            # (a mirrored edge list's target-order records need no sorted target view)
            tv = ecsr.target_view()
            tperm, trowptr = tv.perm, tv.rowptr
            operands |= _ATTN_HAS_TARGET_VIEW
    else:
        nb = L.spt_edge_attn_bwd_workspace_bytes(H, D, Dv, max(F, 1))
    ws = _workspace(nb, dev)
    got = route(operands, ws.numel())
    if got != want:
        raise RuntimeError(f"attention backward (n={n} e={ecsr.e} mode={mode:#x}): prepared for route {want}, "
                           f"the library would take {got}")
    return got, ws, src, tids, tperm, trowptr


def _attn_fwd_call(q, n, H, D, Dv, ecsr, ea, F, ps, scale_mode, scale_a, out, m, z, mode, dev):
    """One spt_edge_attn_fwd_ex_f32; ``ps`` = [Wk, bk, Wq, bq, Wv, bv] (None where absent)."""
    with _timed(f"edge_attn_fwd:{n}:{ecsr.e}"):
        st = _lib.lib.spt_edge_attn_fwd_ex_f32(
            _lib.ptr(q), n, H, D, Dv, _lib.ptr(ecsr.erowptr), _lib.ptr(ecsr.eperm),
            _lib.ptr(ecsr.tgt_sorted), ecsr.e, _lib.ptr(ea), F,
            *[_lib.ptr(t) for t in ps], scale_mode, scale_a, _lib.ptr(out),
            _lib.ptr(m), _lib.ptr(z), mode, _lib.stream_ptr(dev))
    _lib.check(st, "spt_edge_attn_fwd_ex_f32")


def _attn_bwd_call(q, n, H, D, Dv, ecsr, plan, ea, F, ps, scale_mode, scale_a, out, m, z, g, gq, gea,
                   acc, gps, mode, dev, share):
    """One spt_edge_attn_bwd_ex_f32 with the operands of ``plan`` (_attn_bwd_plan); ``gps`` = the
    gradients of ``ps`` in the same order."""
    _, ws, src, tids, tperm, trowptr = plan
    with _timed(f"edge_attn_bwd:{n}:{ecsr.e}"):
        st = _lib.lib.spt_edge_attn_bwd_ex_f32(
            _lib.ptr(q), n, H, D, Dv, _lib.ptr(ecsr.erowptr), _lib.ptr(ecsr.eperm),
            _lib.ptr(ecsr.tgt_sorted), _lib.ptr(src), _lib.ptr(tids), _lib.ptr(tperm),
            _lib.ptr(trowptr), ecsr.e, _lib.ptr(ea), F,
            *[_lib.ptr(t) for t in ps], scale_mode, scale_a, _lib.ptr(out),
            _lib.ptr(m), _lib.ptr(z), _lib.ptr(g), _lib.ptr(gq), _lib.ptr(gea), acc,
            *[_lib.ptr(t) for t in gps], mode, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    if st != 0 and share is not None:
        share.abort()                                # never leave a half-built sum behind
    _lib.check(st, "spt_edge_attn_bwd_ex_f32")


def _at(t, i):
    return None if t is None else t[i]


class _EdgeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, D, scale_mode, scale_a,
                share=None, mode=None):
        _lib.require_cuda(qkv)
        q2 = _f32c(qkv)
        n, ld = q2.shape
        Dv = (ld - 2 * H * D) // H
        if 2 * H * D + H * Dv != ld or ecsr.n != n:
            raise ValueError(f"qkv has shape {tuple(q2.shape)}: not [n={ecsr.n}, 2*H*D + H*Dv]")
        dev = q2.device
        ea = _f32c(edge_attr)
        F = ea.shape[1] if ea is not None else 0
        if ea is not None and ea.shape[0] != ecsr.e:
            raise ValueError("edge_attr rows != number of edges")
        ps = [_f32c(t) for t in (Wk, bk, Wq, bq, Wv, bv)]
        out = torch.empty((n, H * Dv), dtype=torch.float32, device=dev)
        m = torch.empty((n, H), dtype=torch.float32, device=dev)
        z = torch.empty((n, H), dtype=torch.float32, device=dev)
        ctx.mode = mode = _attn_mode(mode)       # resolved: the backward runs in the same mode
        with torch.cuda.device(dev):
            _attn_fwd_call(q2, n, H, D, Dv, ecsr, ea, F, ps, scale_mode, scale_a, out, m, z, mode, dev)
        ctx.save_for_backward(q2, ea, *[t for t in ps if t is not None], out, m, z)
        ctx.present = [t is not None for t in ps]
        ctx.has_ea = ea is not None
        ctx.meta = (ecsr, H, D, Dv, F, scale_mode, scale_a, qkv.dtype,
                    None if edge_attr is None else edge_attr.dtype)
        ctx.share = ctx.rank = None
        if (share is not None and edge_attr is not None and edge_attr.dtype == torch.float32
                and edge_attr.requires_grad and (Wk is not None or Wq is not None or Wv is not None)):
            ctx.share, ctx.rank = share, share.enter(edge_attr)
        return out.to(qkv.dtype)

    @staticmethod
    def backward(ctx, gout):
        ecsr, H, D, Dv, F, scale_mode, scale_a, q_dtype, ea_dtype = ctx.meta
        saved = list(ctx.saved_tensors)
        q2 = saved.pop(0)
        ea = saved.pop(0) if ctx.has_ea else None
        if not ctx.has_ea:
            saved.pop(0)
        ps = [saved.pop(0) if pres else None for pres in ctx.present]
        out, m, z = saved
        n, ld = q2.shape
        dev = q2.device
        g = _f32c(gout)
        gqkv = torch.empty_like(q2)
        share, acc = ctx.share, 0
        if share is not None:
            gea, acc = share.acquire(ctx.rank, ea)       # acc: a later block already started the sum
        else:
            gea = torch.empty_like(ea) if ea is not None else None
        gps = [torch.empty_like(t) if t is not None else None for t in ps]
        plan = _attn_bwd_plan(ecsr, n, H, D, Dv, F, ea is not None and all(ctx.present[0::2]), ctx.mode)
        with torch.cuda.device(dev):
            _attn_bwd_call(q2, n, H, D, Dv, ecsr, plan, ea, F, ps, scale_mode, scale_a, out, m, z, g,
                           gqkv, gea, acc, gps, ctx.mode, dev, share)
        if gea is not None and not (any(ctx.present[0::2])):
            gea = None
        if share is not None:
            gea = share.release(ctx.rank)                # the first block returns the sum
        return (gqkv.to(q_dtype), None, None if gea is None else gea.to(ea_dtype),
                *gps, None, None, None, None, None, None)


def edge_attention(qkv, edge_index, edge_attr=None, k_rpe=None, q_rpe=None, v_rpe=None,
                   num_heads=1, qk_dim=8, scale_mode=0, scale_a=1.0, ea_grad=None):
    """out[s] = sum_e softmax_e(<q_e, k_e>) v_e over the edges leaving s.

    ``qkv`` [N, 2*H*D + C] is the output of the block's qkv Linear;
    ``edge_index`` a [2,E] tensor or an :class:`EdgeCSR`; ``k_rpe`` etc. are
    (weight, bias) pairs of the RPE Linears or None.  Returns [N, C]
    (before out_proj).  ``ea_grad``: an :class:`EdgeAttrGradShare` common to the blocks of a
    stage (their d edge_attr accumulate into one buffer)."""
    ecsr = edge_csr_of(edge_index, qkv.shape[0])

    def wb(p):
        return (None, None) if p is None else (p[0], p[1])

    Wk, bk = wb(k_rpe)
    Wq, bq = wb(q_rpe)
    Wv, bv = wb(v_rpe)
    H, D = int(num_heads), int(qk_dim)
    share = ea_grad if torch.is_grad_enabled() else None
    mode = _attn_mode()                  # resolved once: everything below runs in this word
    split = _matrix_pipe_split(qkv, edge_attr, Wk, Wq, Wv, H, D, mode)
    if split is None:
        padded = _matrix_pipe_pad(qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, D, mode)
        if padded is not None:
            # narrower head layouts (nano: 16 heads of qk_dim 2, value dim 1, 16-D edge encodings)
            # zero-padded to the built (16, 4, 4, 32) shape: the matrix-pipe kernels instead of
            # the generic VALU ones; plain torch ops do the padding, autograd their backward
            qp, eap, wk, bkp, wq, bqp, wv, bvp, dv = padded
            out = _EdgeAttention.apply(qp, ecsr, eap, wk, bkp, wq, bqp, wv, bvp, 16, 4,
                                       int(scale_mode), float(scale_a), None, mode)
            return out.view(out.shape[0], 16, 4)[:, :, :dv].reshape(out.shape[0], 16 * dv)
        return _EdgeAttention.apply(qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, D,
                                    int(scale_mode), float(scale_a), share, mode)
    # wider head layouts (SPT-128: 16 heads of value dim 8; 32 heads) on the matrix-pipe kernels
    G, J, _ = split
    return _EdgeAttentionSplit.apply(qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, G, J,
                                     int(scale_mode), float(scale_a), share, mode)


class _EdgeAttentionSplit(torch.autograd.Function):
    """Wider head layouts on the matrix-pipe kernels, by decomposition.

    The MFMA / edge-lane kernels are built for 16 heads of qk_dim 4 and value dim 4.  Heads are
    independent attention problems and, within a head, the value dims only enter through
    out = sum_e a_e v_e (linear in v; its backward dc = a (<g, v> - <g, out>) is a SUM over the
    value dims), so H = 16 G heads of value dim 4 J decompose EXACTLY into G x J problems of the
    built shape: head group g, value slice j -> columns [q_g | k_g | v_g[:, :, 4j:4j+4]] with the
    matching rows of the RPE weights.  Every pass recomputes the softmax of its head group (the
    price: J x the q / k work).  SPT-128 (KITTI-360: H 16, value dim 8) = 2 passes, 32 heads x 4
    (ScanNet) = 2 passes.

    One autograd node for all passes: the operands of every pass are laid out by ONE gather
    ([G J, N, 192]), the passes write into slabs of one buffer, d edge_attr accumulates in place
    (``acc``) and the q / k / weight gradients of a head group's J passes are summed by one
    reduction each - a per-pass autograd graph (slices, cat, CopySlices, AccumulateGrad) cost
    ~40 five-microsecond launches per block, which is what a train batch's step time is made of."""

    @staticmethod
    def _cols(H, G, J, dev):
        key = (H, G, J, str(dev))
        c = _SPLIT_COLS.get(key)
        if c is None:
            QK, Dv = H * 4, 4 * J
            cols = []
            for gi in range(G):
                for j in range(J):
                    qc = torch.arange(64 * gi, 64 * gi + 64)
                    vc = (2 * QK + (16 * gi + torch.arange(16)).view(16, 1) * Dv + 4 * j
                          + torch.arange(4).view(1, 4)).reshape(64)
                    cols.append(torch.cat([qc, QK + qc, vc]))
            c = _SPLIT_COLS[key] = torch.stack(cols).to(dev)            # [G J, 192]
        return c

    @staticmethod
    def forward(ctx, qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, G, J, scale_mode, scale_a,
                share=None, mode=None):
        _lib.require_cuda(qkv)
        q2 = _f32c(qkv)
        n = q2.shape[0]
        dev = q2.device
        ea = _f32c(edge_attr)
        if ecsr.n != n or ea.shape[0] != ecsr.e:
            raise ValueError("qkv / edge_attr rows do not match the graph")
        P, Dv, F = G * J, 4 * J, 32
        qa = torch.empty((P, n, 192), dtype=torch.float32, device=dev)               # [P, n, 192]
        with torch.cuda.device(dev):
            st = _lib.lib.spt_attn_split_pack_f32(_lib.ptr(q2), n, G, J, _lib.ptr(qa), _lib.stream_ptr(dev))
        _lib.check(st, "spt_attn_split_pack_f32")
        Wk2, Wq2 = _f32c(Wk), _f32c(Wq)
        bk2, bq2 = _f32c(bk), _f32c(bq)
        Wva = _f32c(Wv).view(G, 16, J, 4, F).permute(0, 2, 1, 3, 4).contiguous()      # [G, J, 64, F]
        bva = None if bv is None else _f32c(bv).view(G, 16, J, 4).permute(0, 2, 1, 3).contiguous()
        oa = torch.empty((P, n, 64), dtype=torch.float32, device=dev)
        m = torch.empty((P, n, 16), dtype=torch.float32, device=dev)
        z = torch.empty((P, n, 16), dtype=torch.float32, device=dev)
        ctx.mode = mode = _attn_mode(mode)
        with torch.cuda.device(dev):
            for gi in range(G):
                cs = slice(64 * gi, 64 * gi + 64)
                for j in range(J):
                    p = gi * J + j
                    ps = [Wk2[cs], _at(bk2, cs), Wq2[cs], _at(bq2, cs), Wva[gi, j], _at(bva, (gi, j))]
                    _attn_fwd_call(qa[p], n, 16, 4, 4, ecsr, ea, F, ps, scale_mode, scale_a, oa[p], m[p],
                                   z[p], mode, dev)
        ctx.save_for_backward(qa, ea, Wk2, Wq2, Wva, oa, m, z,
                              *[t for t in (bk2, bq2, bva) if t is not None])
        ctx.has_b = [t is not None for t in (bk2, bq2, bva)]
        ctx.meta = (ecsr, H, G, J, scale_mode, scale_a, qkv.dtype, edge_attr.dtype)
        ctx.share = ctx.rank = None
        if share is not None and edge_attr.dtype == torch.float32 and edge_attr.requires_grad:
            ctx.share, ctx.rank = share, share.enter(edge_attr)
        out = oa.view(G, J, n, 16, 4).permute(2, 0, 3, 1, 4).reshape(n, H * Dv)
        return out.to(qkv.dtype)

    @staticmethod
    def backward(ctx, gout):
        ecsr, H, G, J, scale_mode, scale_a, q_dtype, ea_dtype = ctx.meta
        saved = list(ctx.saved_tensors)
        qa, ea, Wk2, Wq2, Wva, oa, m, z = saved[:8]
        rest = saved[8:]
        bk2, bq2, bva = [rest.pop(0) if h else None for h in ctx.has_b]
        P, n = qa.shape[0], qa.shape[1]
        dev, F, Dv, QK = qa.device, 32, 4 * J, 4 * H
        ga = _f32c(gout).view(n, G, 16, J, 4).permute(1, 3, 0, 2, 4).contiguous().view(P, n, 64)
        gqa = torch.empty_like(qa)
        share, acc = ctx.share, 0
        if share is not None:
            gea, acc = share.acquire(ctx.rank, ea)
        else:
            gea = torch.empty_like(ea)
        gWk = torch.empty((P, 64, F), dtype=torch.float32, device=dev)
        gWq = torch.empty_like(gWk)
        gWv = torch.empty_like(gWk)
        gbk = torch.empty((P, 64), dtype=torch.float32, device=dev) if bk2 is not None else None
        gbq = torch.empty((P, 64), dtype=torch.float32, device=dev) if bq2 is not None else None
        gbv = torch.empty((P, 64), dtype=torch.float32, device=dev) if bva is not None else None
        plan = _attn_bwd_plan(ecsr, n, 16, 4, 4, F, True, ctx.mode)
        with torch.cuda.device(dev):
            for gi in range(G):
                cs = slice(64 * gi, 64 * gi + 64)
                for j in range(J):
                    p = gi * J + j
                    ps = [Wk2[cs], _at(bk2, cs), Wq2[cs], _at(bq2, cs), Wva[gi, j], _at(bva, (gi, j))]
                    gps = [gWk[p], _at(gbk, p), gWq[p], _at(gbq, p), gWv[p], _at(gbv, p)]
                    _attn_bwd_call(qa[p], n, 16, 4, 4, ecsr, plan, ea, F, ps, scale_mode, scale_a, oa[p],
                                   m[p], z[p], ga[p], gqa[p], gea, acc, gps, ctx.mode, dev, share)
                    acc = 1
        # q / k (and their encoders') gradients: the sum over a head group's J value slices
        gqkv = torch.empty((n, 2 * QK + H * Dv), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_attn_split_grad_f32(_lib.ptr(gqa), n, G, J, _lib.ptr(gqkv), _lib.stream_ptr(dev))
        _lib.check(st, "spt_attn_split_grad_f32")

        def over_j(t, tail):
            if t is None:
                return None
            t = t.view(G, J, *tail)
            return (t.sum(1) if J > 1 else t[:, 0]).reshape(G * tail[0], *tail[1:])

        def value_rows(t, tail):                       # [G, J, 16, 4, ...] -> rows h * Dv + 4 j + d
            if t is None:
                return None
            t = t.view(G, J, 16, 4, *tail)
            return t.permute(0, 2, 1, 3, *range(4, 4 + len(tail))).reshape(H * Dv, *tail)

        if share is not None:
            gea = share.release(ctx.rank)
        return (gqkv.to(q_dtype), None, None if gea is None else gea.to(ea_dtype),
                over_j(gWk, (64, F)), over_j(gbk, (64,)), over_j(gWq, (64, F)), over_j(gbq, (64,)),
                value_rows(gWv, (F,)), value_rows(gbv, ()), None, None, None, None, None, None, None)


_SPLIT_COLS = {}


PAD_MIN_EDGES = 1 << 16        # below that the generic kernels are a few microseconds anyway


def _matrix_pipe_pad(qkv, ecsr, edge_attr, Wk, bk, Wq, bq, Wv, bv, H, D, mode=None):
    """Operands of a head layout NARROWER than the built (16, 4, 4, 32) one, zero-padded to it
    (H = 16, qk_dim <= 4, value dim <= 4, in_rpe_dim <= 32, all three RPE encoders, a
    matrix-pipe precision active, enough edges to matter); None otherwise.  Exact: padded q / k
    dims add zero to every dot product, padded value dims and edge-encoding columns meet zero
    weights, the padded output dims are dropped."""
    if H != 16 or D > 4 or edge_attr is None or Wk is None or Wq is None or Wv is None:
        return None
    F = edge_attr.shape[1]
    C = qkv.shape[1] - 2 * H * D
    if C <= 0 or C % H or F > 32 or ecsr.e < PAD_MIN_EDGES:
        return None
    Dv = C // H
    if Dv > 4 or (D == 4 and Dv == 4 and F == 32):
        return None
    if qkv.dtype != torch.float32 or edge_attr.dtype != torch.float32:
        return None
    if (_attn_mode(mode) & 3) == 0:
        return None
    n, e = qkv.shape[0], edge_attr.shape[0]
    pad = torch.nn.functional.pad

    def heads(t, d):                                 # [rows, H * d] -> [rows, H * 4]
        return t if d == 4 else pad(t.reshape(t.shape[0], H, d), (0, 4 - d)).reshape(t.shape[0], H * 4)

    def enc(w, b, d):                                # ([H d, F], [H d]) -> ([H 4, 32], [H 4])
        w = pad(w.reshape(H, d, F), (0, 32 - F, 0, 4 - d)).reshape(H * 4, 32)
        b = None if b is None else pad(b.reshape(H, d), (0, 4 - d)).reshape(H * 4)
        return w.contiguous(), b
    q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
    qp = torch.cat([heads(q, D), heads(k, D), heads(v, Dv)], dim=1)
    eap = edge_attr if F == 32 else pad(edge_attr, (0, 32 - F))
    wk, bkp = enc(Wk, bk, D)
    wq, bqp = enc(Wq, bq, D)
    wv, bvp = enc(Wv, bv, Dv)
    return qp, eap, wk, bkp, wq, bqp, wv, bvp, Dv


def _matrix_pipe_split(qkv, edge_attr, Wk, Wq, Wv, H, D, mode=None):
    """(G, J, Dv) when a head layout other than the built (16, 4, 4) decomposes into G x J passes
    of it (H = 16 G, qk_dim 4, value dim 4 J, in_rpe_dim 32, all three RPE encoders, a matrix-pipe
    precision active); None for the built shape itself and for everything else (generic kernels)."""
    if D != 4 or H % 16 or edge_attr is None or Wk is None or Wq is None or Wv is None:
        return None
    if edge_attr.shape[1] != 32:
        return None
    C = qkv.shape[1] - 2 * H * D
    if C <= 0 or C % H:
        return None
    Dv = C // H
    if Dv % 4 or (H == 16 and Dv == 4):
        return None
    if (_attn_mode(mode) & 3) == 0:
        return None
    return H // 16, Dv // 4, Dv


# ---------------------------------------------------------------------------
# Dense Linear on tall-skinny operands (plumbing over rocBLAS / hipBLASLt)
# ---------------------------------------------------------------------------
_DW_CHUNK = 32768
_SKINNY_MIN_ROWS = 4096


def _skinny_ok(x, weight):
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and x.dim() == 2 and x.shape[0] >= _SKINNY_MIN_ROWS
            and _lib.lib.spt_skinny_linear_supported(weight.shape[1], weight.shape[0]))


def _skinny_launch(x, weight, bias, mode=-1):
    """y = x W^T + b on the MFMA skinny-GEMM kernel (csrc/skinny_linear.hip); ``mode``: the matrix
    mode word of the call (``precision.skinny_mode()``; -1 = the library's default)."""
    x, weight, bias = _dense(x), _dense(weight), _dense(bias)
    rows, k = x.shape
    n = weight.shape[0]
    y = torch.empty((rows, n), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = _lib.lib.spt_skinny_linear_pre_m_f32(
            _lib.ptr(x), rows, k, _lib.ptr(weight), _lib.ptr(bias), n, _lib.ptr(y),
            None, None, None, None, 1, None, int(mode), _lib.stream_ptr(x.device))
    _lib.check(st, "spt_skinny_linear_pre_m_f32")
    return y


def _input_grad(g, weight, mode=-1):
    """dX = G W of a Linear (``weight`` [N_out, N_in] as the layer holds it): the skinny kernel reads
    the weight transposed while it stages the slab (``spt_skinny_linear_wt_f32``) - no transposed
    copy per backward call -, else the transposed copy on the same kernel, else the library."""
    n_out, n_in = weight.shape
    if (g.is_cuda and g.dtype == torch.float32 and weight.dtype == torch.float32 and g.dim() == 2
            and g.shape[0] >= _SKINNY_MIN_ROWS and n_in % 4 == 0 and n_in >= 64
            and _lib.lib.spt_skinny_linear_supported(n_out, n_in)):
        g = _dense(g)
        w = _dense(weight.detach())
        rows = g.shape[0]
        y = torch.empty((rows, n_in), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            st = _lib.lib.spt_skinny_linear_wt_m_f32(_lib.ptr(g), rows, n_out, _lib.ptr(w), n_in,
                                                     _lib.ptr(y), int(mode), _lib.stream_ptr(g.device))
        _lib.check(st, "spt_skinny_linear_wt_m_f32")
        return y
    wt = weight.detach().t().contiguous()           # [K, N]: dX = G (W^T)^T
    return _skinny_launch(g, wt, None, mode) if _skinny_ok(g, wt) else g @ weight


def _dw_batched(g, x):
    """dW = G^T X reduces over millions of rows into a <=192x192 output, a shape the
    library runs on a handful of workgroups - so it is issued as a BATCHED GEMM over row
    chunks (thousands of workgroups) followed by a small sum."""
    n = x.shape[0]
    nb = n // _DW_CHUNK
    main = nb * _DW_CHUNK
    gw = None
    if nb > 0:
        gm = g[:main].reshape(nb, _DW_CHUNK, g.shape[1])
        xm = x[:main].reshape(nb, _DW_CHUNK, x.shape[1])
        gw = torch.bmm(gm.transpose(1, 2), xm).sum(0)
    if main < n:
        tail = g[main:].t() @ x[main:]
        gw = tail if gw is None else gw + tail
    return gw


def _skinny_dw_ok(g, x):
    return (x.is_cuda and x.dtype == torch.float32 and g.dtype == torch.float32
            and x.shape[0] >= _SKINNY_MIN_ROWS
            and _lib.lib.spt_skinny_dw_supported(x.shape[1], g.shape[1]))


def _skinny_dw(g, x, want_bias=False, mode=-1):
    """dW = G^T X (and, from the same pass, db = column sums of G) on the MFMA kernel of
    csrc/skinny_linear.hip (per-wave partials, fixed-order sum)."""
    g, x = _dense(g), _dense(x.detach())
    rows, k = x.shape
    n = g.shape[1]
    gw = torch.empty((n, k), dtype=torch.float32, device=x.device)
    gb = torch.empty(n, dtype=torch.float32, device=x.device) if want_bias else None
    nb = _lib.lib.spt_skinny_dw_workspace_bytes(k, n)
    ws = _workspace(nb, x.device)
    with torch.cuda.device(x.device):
        st = _lib.lib.spt_skinny_dw_pre_m_f32(_lib.ptr(g), _lib.ptr(x), rows, n, k, _lib.ptr(gw),
                                              _lib.ptr(gb), None, None, None, None, 1, int(mode),
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
    _lib.check(st, "spt_skinny_dw_pre_m_f32")
    return (gw, gb) if want_bias else gw


_BWD_ROUTE = {"fused": 0, "split": 0}


def skinny_bwd_fused(on=None):
    """Switch of the one-pass backward of the attention blocks' Linears (dX, dW and db from one read
    of the gradient, csrc/skinny_linear.hip: ``spt_skinny_linear_bwd_m_f32``); default on,
    ``SPT_SKINNY_BWD_FUSED=0`` in the environment turns it off.  Returns the previous setting."""
    return bool(_lib.lib.spt_skinny_bwd_fused(-1 if on is None else int(bool(on))))


def skinny_bwd_route_counts():
    """Calls of the tall Linears' backward so far that took the one-pass entry (``fused``) and the
    dX / dW launches (``split``) - the route query of the tests."""
    return dict(_BWD_ROUTE)


def _skinny_bwd_ok(g, x, weight, num_graphs, mode):
    return bool(x.is_cuda and x.dtype == torch.float32 and g.dtype == torch.float32
                and weight.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= _SKINNY_MIN_ROWS
                and _lib.lib.spt_skinny_bwd_fused(-1)
                and _lib.lib.spt_skinny_linear_bwd_supported(x.shape[1], g.shape[1], int(num_graphs),
                                                             int(mode)))


def _skinny_bwd(g, x, weight, want_bias, mode, pre=None):
    """(gx, gw, gb) of y = x W^T + b from one pass over (g, x); ``pre`` = (am, scale, bias, batch, B):
    x normalised on its way in (the folded pre-norm), gx then is the gradient of the normalised rows."""
    g, x, w = _dense(g), _dense(x.detach()), _dense(weight.detach())
    rows, k = x.shape
    n = g.shape[1]
    dev = x.device
    gx = torch.empty((rows, k), dtype=torch.float32, device=dev)
    gw = torch.empty((n, k), dtype=torch.float32, device=dev)
    gb = torch.empty(n, dtype=torch.float32, device=dev) if want_bias else None
    am, sc, pb, batch, B = pre if pre is not None else (None, None, None, None, 1)
    ws = _workspace(_lib.lib.spt_skinny_linear_bwd_workspace_bytes(k, n), dev)
    with torch.cuda.device(dev):
        st = _lib.lib.spt_skinny_linear_bwd_m_f32(
            _lib.ptr(g), _lib.ptr(x), _lib.ptr(w), rows, n, k, _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb),
            _lib.ptr(am), _lib.ptr(sc), _lib.ptr(pb), _lib.ptr(batch), int(B), int(mode), _lib.ptr(ws),
            ws.numel(), _lib.stream_ptr(dev))
    _lib.check(st, "spt_skinny_linear_bwd_m_f32")
    _BWD_ROUTE["fused"] += 1
    return gx, gw, gb


class _TallLinear(torch.autograd.Function):
    """y = x W^T (+ b) for [rows >> features] operands.  Forward and dX run on the
    hand-written skinny-GEMM kernel when the shape is built (K in {32,64,128,192},
    N % 64 == 0 - the attention block's qkv / out_proj), else on the library; dW on the
    skinny dW kernel (K in {32, 64}) or a batched library GEMM over row chunks.  Where both dX and
    dW are wanted and the one-pass backward is built (K = 64, N in {64, 192}, a bf16 matrix mode,
    ``skinny_bwd_fused``) one launch reads the gradient once for dX, dW and db."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.smode = _precision.skinny_mode()      # the backward runs in the mode of the forward
        if _skinny_ok(x, weight):
            return _skinny_launch(x.detach(), weight.detach(), None if bias is None else bias.detach(),
                                  ctx.smode)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        # (dense operands on the library routes below the row floor too: a GEMM on a transposed
        # or strided view takes another kernel and gives other bits than on its dense copy)
        g, x, weight = _dense(g), _dense(x.detach()), _dense(weight.detach())
        if (x.is_cuda and x.dtype == torch.float32 and g.dtype == torch.float32
                and weight.dtype == torch.float32 and x.shape[0] >= _SKINNY_MIN_ROWS
                and _lib.lib.spt_narrow_linear_bwd_supported(x.shape[1], g.shape[1])):
            # narrow head: dX, dW and db from one pass over (x, g)
            xc, wc = x, weight
            rows, k = xc.shape
            n = g.shape[1]
            dev = xc.device
            gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
            gw = torch.empty((n, k), dtype=torch.float32, device=dev)
            gb = torch.empty(n, dtype=torch.float32, device=dev) if ctx.has_bias else None
            nb = _lib.lib.spt_narrow_linear_bwd_workspace_bytes(k, n)
            ws = _workspace(nb, dev)
            with torch.cuda.device(dev):
                st = _lib.lib.spt_narrow_linear_bwd_f32(
                    _lib.ptr(g), _lib.ptr(xc), _lib.ptr(wc), rows, n, k, _lib.ptr(gx),
                    _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
            _lib.check(st, "spt_narrow_linear_bwd_f32")
            return gx, gw, gb
        gx = None
        smode = getattr(ctx, "smode", -1)
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and _skinny_bwd_ok(g, x, weight, 1, smode):
            return _skinny_bwd(g, x, weight, want_gb, smode)
        _BWD_ROUTE["split"] += 1
        if ctx.needs_input_grad[0]:
            gx = _input_grad(g, weight, smode)
        gw = gb = None
        if ctx.needs_input_grad[1]:
            if _skinny_dw_ok(g, x):
                gw = _skinny_dw(g, x, want_gb, smode)
                if want_gb:
                    gw, gb = gw
            else:
                gw = _dw_batched(g, x) if x.shape[0] >= 4 * _DW_CHUNK else g.t() @ x
        if want_gb and gb is None:
            gb = g.sum(0)
        return gx, gw, gb


def linear(x, weight, bias=None):
    """``nn.Linear`` forward for tall-skinny operands (see _TallLinear); small or
    unsupported inputs go straight to the library."""
    if x.dim() != 2 or not x.is_cuda or x.shape[0] < _SKINNY_MIN_ROWS:
        return torch.nn.functional.linear(x, weight, bias)
    return _TallLinear.apply(x, weight, bias)


class _ResidualLinear(torch.autograd.Function):
    """y = residual + (x W^T + b): a transformer block's `shortcut + out_proj(.)`
    (src/nn/transformer.py:231-234, src/nn/attention.py:318-319) with the add in the skinny
    kernel's epilogue (bitwise `residual + linear(x)`).  The residual's gradient is the incoming
    gradient itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.smode = _precision.skinny_mode()
        xd, wd = _dense(x.detach()), _dense(weight.detach())
        bd = None if bias is None else _dense(bias.detach(), torch.float32)
        res = _dense(residual.detach())          # (named: a copy must outlive the launch)
        rows, k = xd.shape
        n = wd.shape[0]
        y = torch.empty((rows, n), dtype=torch.float32, device=xd.device)
        with torch.cuda.device(xd.device):
            st = _lib.lib.spt_skinny_linear_pre_m_f32(
                _lib.ptr(xd), rows, k, _lib.ptr(wd), _lib.ptr(bd), n, _lib.ptr(y),
                None, None, None, None, 1, _lib.ptr(res), ctx.smode, _lib.stream_ptr(xd.device))
        _lib.check(st, "spt_skinny_linear_pre_m_f32")
        return y

    @staticmethod
    def backward(ctx, g):
        gx, gw, gb = _TallLinear.backward(ctx, g)
        return gx, gw, gb, g


_FUSE_PRENORM = os.environ.get("SPT_FUSE_PRENORM", "1") != "0"


def fuse_prenorm(on=None):
    """Switch of the folded pre-norm / residual route of the transformer blocks (default on;
    ``SPT_FUSE_PRENORM=0`` in the environment turns it off).  Returns the previous setting."""
    global _FUSE_PRENORM
    prev = _FUSE_PRENORM
    if on is not None:
        _FUSE_PRENORM = bool(on)
    return prev


def linear_residual_ok(residual, weight):
    """Whether ``linear_residual`` runs fused for a Linear with this weight whose output is
    added to ``residual`` [rows, N]: tall f32 rows, (K, N) built."""
    return bool(_FUSE_PRENORM and residual.dim() == 2 and residual.is_cuda
                and residual.dtype == torch.float32 and weight.dtype == torch.float32
                and residual.shape[0] >= _SKINNY_MIN_ROWS and residual.shape[1] == weight.shape[0]
                and _lib.lib.spt_skinny_pre_supported(weight.shape[1], weight.shape[0], 1))


def linear_residual(x, weight, bias, residual):
    """``residual + F.linear(x, weight, bias)`` with the add folded into the Linear's kernel where
    the shape is built (tall f32 operands, K in {32, 64, 128}, N a multiple of 64)."""
    if (x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] == residual.shape[0]
            and linear_residual_ok(residual, weight)):
        return _ResidualLinear.apply(x, weight, bias, residual)
    return residual + linear(x, weight, bias)


class _NormLinear(torch.autograd.Function):
    """qkv = Linear(GraphNorm(x)) with the norm applied INSIDE the Linear's read of x
    (`spt_graphnorm_stats_f32` + `spt_skinny_linear_pre_f32`): the pre-norm of a transformer block
    (src/nn/transformer.py:231-234) without the normalised [rows, C] tensor ever being written.
    Returns ``(y, x_res)``: ``x_res`` is x itself, handed back so that the block's residual
    branch hangs on THIS node - the backward then receives both gradients of x and the norm's
    backward kernel adds them in its own pass (`spt_graphnorm_bwd_acc_f32`), instead of autograd
    summing two [rows, C] tensors with one more launch.  Values are bitwise those of
    ``linear(graph_norm(x))``."""

    @staticmethod
    def forward(ctx, x, batch, num_graphs, gn_w, gn_b, gn_a, eps, weight, bias):
        _lib.require_cuda(x)
        xd = _dense(x.detach())
        rows, d = xd.shape
        dev = xd.device
        B = int(num_graphs)
        batch = _dense(batch, torch.int64, 8)
        w, b, a = (_dense(t.detach(), torch.float32) for t in (gn_w, gn_b, gn_a))
        wd = _dense(weight.detach())
        bd = None if bias is None else _dense(bias.detach(), torch.float32)
        n = wd.shape[0]
        mean, rstd, am, sc = (torch.empty((B, d), dtype=torch.float32, device=dev) for _ in range(4))
        y = torch.empty((rows, n), dtype=torch.float32, device=dev)
        nb = _lib.lib.spt_graphnorm_workspace_bytes(rows, d, B)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_graphnorm_stats_f32(
                _lib.ptr(xd), _lib.ptr(batch), rows, d, B, _lib.ptr(w), _lib.ptr(a), float(eps),
                _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(am), _lib.ptr(sc), _lib.ptr(ws),
                ws.numel(), _lib.stream_ptr(dev))
            _lib.check(st, "spt_graphnorm_stats_f32")
            smode = _precision.skinny_mode()
            st = _lib.lib.spt_skinny_linear_pre_m_f32(
                _lib.ptr(xd), rows, d, _lib.ptr(wd), _lib.ptr(bd), n, _lib.ptr(y), _lib.ptr(am),
                _lib.ptr(sc), _lib.ptr(b), _lib.ptr(batch), B, None, smode, _lib.stream_ptr(dev))
        _lib.check(st, "spt_skinny_linear_pre_m_f32")
        ctx.save_for_backward(xd, batch, w, b, a, mean, rstd, am, sc, wd)
        ctx.meta = (B, bias is not None)
        ctx.smode = smode                          # the backward runs in the mode of the forward
        # an unused output arrives as None in the backward instead of a dense zero [rows, C]
        # tensor that the norm's backward kernel would read for nothing
        ctx.set_materialize_grads(False)
        return y, x

    @staticmethod
    def backward(ctx, gy, gres):
        xd, batch, w, b, a, mean, rstd, am, sc, wd = ctx.saved_tensors
        B, has_bias = ctx.meta
        if gy is None:                       # only the residual branch was used
            return gres, None, None, None, None, None, None, None, None
        rows, d = xd.shape
        n = wd.shape[0]
        dev = xd.device
        gy = _dense(gy)
        if ctx.needs_input_grad[7] and _skinny_bwd_ok(gy, xd, wd, B, ctx.smode):
            # gradient wrt the normalised rows, weight / bias gradient against the rows normalised
            # on the fly: one pass over (gy, x)
            gxn, gw, gb = _skinny_bwd(gy, xd, wd, has_bias, ctx.smode, (am, sc, b, batch, B))
        else:
            _BWD_ROUTE["split"] += 1
            # gradient wrt the normalised rows: dX of the Linear
            gxn = _input_grad(gy, wd, ctx.smode)
            # weight / bias gradient against the rows normalised on the fly
            gw = torch.empty((n, d), dtype=torch.float32, device=dev)
            gb = torch.empty(n, dtype=torch.float32, device=dev) if has_bias else None
            ws = _workspace(_lib.lib.spt_skinny_dw_workspace_bytes(d, n), dev)
            with torch.cuda.device(dev):
                st = _lib.lib.spt_skinny_dw_pre_m_f32(
                    _lib.ptr(gy), _lib.ptr(xd), rows, n, d, _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(am),
                    _lib.ptr(sc), _lib.ptr(b), _lib.ptr(batch), B, ctx.smode, _lib.ptr(ws), ws.numel(),
                    _lib.stream_ptr(dev))
            _lib.check(st, "spt_skinny_dw_pre_m_f32")
        # the norm's backward, with the residual branch's gradient added in its apply pass
        gx = torch.empty_like(xd)
        g_w, g_b, g_a = (torch.empty(d, dtype=torch.float32, device=dev) for _ in range(3))
        if gres is not None:
            gres = _dense(gres)
        ws = _workspace(_lib.lib.spt_graphnorm_workspace_bytes(rows, d, B), dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_graphnorm_bwd_acc_f32(
                _lib.ptr(xd), _lib.ptr(gxn), _lib.ptr(batch), rows, d, B, _lib.ptr(w), _lib.ptr(b),
                _lib.ptr(a), _lib.ptr(mean), _lib.ptr(rstd), 1.0, _lib.ptr(gres), _lib.ptr(gx),
                _lib.ptr(g_w), _lib.ptr(g_b), _lib.ptr(g_a), _lib.ptr(ws), ws.numel(),
                _lib.stream_ptr(dev))
        _lib.check(st, "spt_graphnorm_bwd_acc_f32")
        return gx, None, None, g_w, g_b, g_a, None, gw, gb


def norm_linear_ok(x, batch, num_graphs, weight):
    """Whether ``norm_linear`` runs fused: tall f32 rows, a built (K, N), few graphs."""
    if not _FUSE_PRENORM or (batch is not None and num_graphs is None):
        return False
    B = 1 if batch is None else int(num_graphs)
    return bool(x.dim() == 2 and x.is_cuda and x.dtype == torch.float32
                and weight.dtype == torch.float32 and x.shape[0] >= _SKINNY_MIN_ROWS
                and _lib.lib.spt_skinny_pre_supported(x.shape[1], weight.shape[0], B)
                and _lib.lib.spt_skinny_dw_supported(x.shape[1], weight.shape[0]))


_BCHK_ATTR = "_spt_batch_checked"


def _check_batch_ids(batch, B):
    """The folded pre-norm kernels index LDS tables by ``batch[row]``: ids outside [0, B) must fail
    here, as they do on the unfused ``graph_norm`` route, not read tables out of range.  One
    memoised device reduction per batch vector (none when its maker left the host ranges)."""
    if batch is None or _host_ptr(batch, B) is not None:
        return
    key = (batch._version, int(B), batch.data_ptr(), batch.numel())
    if getattr(batch, _BCHK_ATTR, None) == key:
        return
    if batch.numel():
        lo, hi = torch.aminmax(batch)
        if int(lo) < 0 or int(hi) >= int(B):
            raise ValueError(f"graph ids of `batch` must lie in [0, {int(B)}): found [{int(lo)}, {int(hi)}]")
    try:
        setattr(batch, _BCHK_ATTR, key)
    except Exception:
        pass


def norm_linear(x, batch, num_graphs, gn_weight, gn_bias, gn_mean_scale, eps, weight, bias):
    """``(linear(graph_norm(x, batch), weight, bias), x_res)`` - see ``_NormLinear``.  Callers
    check ``norm_linear_ok`` first."""
    B = 1 if batch is None else int(num_graphs)
    _check_batch_ids(batch, B)
    return _NormLinear.apply(x, batch, B, gn_weight, gn_bias, gn_mean_scale, float(eps), weight, bias)


# ---------------------------------------------------------------------------
# Cross-entropy of the heads' logits (csrc/loss.hip)
# ---------------------------------------------------------------------------
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        _lib.require_cuda(logits, target)
        lg = _f32c(logits)
        tg = _dense(target, torch.int64, 8)
        rows, c = lg.shape
        dev = lg.device
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)          # loss | count
        nb = _lib.lib.spt_cross_entropy_workspace_bytes(rows)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_cross_entropy_fwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), rows, c, int(ignore_index), _lib.ptr(lse),
                _lib.ptr(out), _lib.ptr(out[1:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "spt_cross_entropy_fwd_f32")
        ctx.save_for_backward(lg, tg, lse, out)
        ctx.meta = (int(ignore_index), logits.dtype)
        return out[0].to(logits.dtype)

    @staticmethod
    def backward(ctx, gout):
        lg, tg, lse, out = ctx.saved_tensors
        ignore_index, dtype = ctx.meta
        rows, c = lg.shape
        dev = lg.device
        g = _dense(gout.detach().reshape(1), torch.float32, 4)
        glog = torch.empty_like(lg)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_cross_entropy_bwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), _lib.ptr(lse), rows, c, ignore_index, _lib.ptr(g),
                _lib.ptr(out[1:]), _lib.ptr(glog), _lib.stream_ptr(dev))
        _lib.check(st, "spt_cross_entropy_bwd_f32")
        return glog.to(dtype), None, None


def cross_entropy(logits, target, ignore_index=-100, weight=None):
    """``torch.nn.functional.cross_entropy(logits, target, weight=..., ignore_index=...)`` (mean
    reduction) for [rows, C <= 32] logits on the HIP kernels; anything else goes to torch.  With
    class weights (``weighted_loss: True``) the mean is over ``sum w[target]`` (index mode of the
    histogram-loss kernels below)."""
    if weight is not None:
        return _hist_loss(logits, target, weight, HL_INDEX, ignore_index, None)
    if (logits.is_cuda and logits.dim() == 2 and 1 <= logits.shape[1] <= 32
            and logits.shape[0] >= 1 and target.dim() == 1):
        return _CrossEntropy.apply(logits, target, ignore_index)
    return torch.nn.functional.cross_entropy(logits, target, ignore_index=ignore_index)


# ---------------------------------------------------------------------------
# Class-weighted CE on label histograms + histogram confusion matrix (csrc/loss.hip): the
# reference's default criterion (loss_type 'ce_kl', weighted_loss True) and its metric
# ---------------------------------------------------------------------------
HL_INDEX, HL_DOMINANT, HL_HISTOGRAM = 0, 1, 2
_HL_MODES = {"index": HL_INDEX, "dominant": HL_DOMINANT, "histogram": HL_HISTOGRAM}


def _check_hist(logits, target, mode):
    if logits.dim() != 2 or not logits.is_floating_point():
        raise ValueError(f"logits must be a floating [rows, C] tensor, got {tuple(logits.shape)}")
    c = logits.shape[1]
    if target.is_floating_point() or target.shape[0] != logits.shape[0]:
        raise ValueError("the target must be an integer tensor with one row per logits row")
    if mode == HL_INDEX:
        if target.dim() != 1:
            raise ValueError(f"index targets are [rows], got {tuple(target.shape)}")
    elif target.dim() != 2 or target.shape[1] not in (c, c + 1):
        raise ValueError(f"a label histogram for {c} classes has {c} or {c + 1} (void) columns, "
                         f"got {tuple(target.shape)}")


def _hist_loss_torch(logits, target, weight, mode, ignore_index):
    """The closed forms of the kernels as a torch composition (CPU tensors, C > 32): fixed output
    sizes only - no ``where(mask)``, no ``repeat_interleave`` - so nothing waits on the host."""
    z = logits
    c = z.shape[1]
    w = torch.ones(c, dtype=z.dtype, device=z.device) if weight is None else weight.to(z.dtype)
    lse = torch.logsumexp(z, dim=1)
    nan = torch.full((), float("nan"), dtype=z.dtype, device=z.device)
    if mode == HL_HISTOGRAM:
        hw = target[:, :c].to(z.dtype) * w
        num = torch.where(hw != 0, hw * (lse[:, None] - z), torch.zeros_like(z)).sum()
        den = target.sum().to(z.dtype)
        bad = (target < 0).any()
    else:
        if mode == HL_DOMINANT:
            t, ignore_index, bad = target.argmax(dim=1), c, (target < 0).any()
        else:
            t = target
            bad = ((t != ignore_index) & ((t < 0) | (t >= c))).any()
        tc = t.clamp(0, c - 1)
        wt = w[tc] * ((t != ignore_index) & (t >= 0) & (t < c)).to(z.dtype)
        num = (wt * (lse - z.gather(1, tc[:, None])[:, 0])).sum()
        den = wt.sum()
    return torch.where(bad, nan, num) / den


class _HistLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, mode, ignore_index, confmat):
        _lib.require_cuda(logits, target, weight, confmat)
        lg = _f32c(logits)
        tg = _dense(target, torch.int64, 8)
        wt = _f32c(weight)
        rows, c = lg.shape
        ncols = tg.shape[1] if tg.dim() == 2 else 0
        dev = lg.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        den = torch.empty(1, dtype=torch.float64, device=dev)
        ws = _workspace(_lib.lib.spt_cross_entropy_workspace_bytes(rows), dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_hist_loss_fwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), rows, c, ncols, mode, int(ignore_index), _lib.ptr(wt),
                _lib.ptr(loss), _lib.ptr(den), _lib.ptr(confmat), _lib.ptr(ws), ws.numel(),
                _lib.stream_ptr(dev))
        _lib.check(st, "spt_hist_loss_fwd_f32")
        ctx.save_for_backward(lg, tg, wt, den)
        ctx.meta = (mode, int(ignore_index), logits.dtype)
        return loss[0].to(logits.dtype)

    @staticmethod
    def backward(ctx, gout):
        lg, tg, wt, den = ctx.saved_tensors
        mode, ignore_index, dtype = ctx.meta
        rows, c = lg.shape
        ncols = tg.shape[1] if tg.dim() == 2 else 0
        dev = lg.device
        g = _dense(gout.detach().reshape(1), torch.float32, 4)
        glog = torch.empty_like(lg)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_hist_loss_bwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), rows, c, ncols, mode, ignore_index, _lib.ptr(wt),
                _lib.ptr(g), _lib.ptr(den), _lib.ptr(glog), _lib.stream_ptr(dev))
        _lib.check(st, "spt_hist_loss_bwd_f32")
        return glog.to(dtype), None, None, None, None, None


def _hist_loss(logits, target, weight, mode, ignore_index, confmat):
    _check_hist(logits, target, mode)
    c = logits.shape[1]
    if weight is not None and tuple(weight.shape) != (c,):
        raise ValueError(f"class weights must be [{c}], got {tuple(weight.shape)}")
    if confmat is not None and (mode == HL_INDEX or confmat.dtype != torch.int64
                                or tuple(confmat.shape) != (c, c) or not confmat.is_contiguous()):
        raise ValueError(f"the fused confusion matrix is a contiguous int64 [{c}, {c}] buffer "
                         "and needs histogram targets")
    if logits.is_cuda and c <= 32 and logits.shape[0] >= 1:
        return _HistLoss.apply(logits, target, weight, mode, ignore_index, confmat)
    if confmat is not None:
        histogram_confusion_matrix(logits.detach(), target, c, out=confmat)
    return _hist_loss_torch(logits, target, weight, mode, ignore_index)


def histogram_loss(logits, y_hist, weight=None, mode="histogram", confmat=None):
    """Class-weighted cross-entropy of [rows, C] logits against int64 label histograms
    ``y_hist`` [rows, C or C + 1] (last column void when C + 1), differentiable in ``logits``:

    ``mode="histogram"``: ``loss_with_target_histogram(CrossEntropyLoss(weight, ignore_index=C),
    logits, y_hist)`` of the reference (src/utils/loss.py:25-38) in closed form,
    ``sum h[r, c] w[c] (lse_r - z[r, c]) / sum h`` (the void column counts in the denominator only);
    ``mode="dominant"``: ``CrossEntropyLoss(weight, ignore_index=C)(logits, y_hist.argmax(1))``.

    ``confmat``: optional int64 [C, C] buffer; the confusion matrix of ``argmax logits`` against
    the histograms is ADDED to it by the same pass (a validation step's loss and metric together).
    CUDA tensors with C <= 32 run on the HIP kernels (no host synchronisation: the call can be
    captured into a graph); CPU tensors and wider heads take a sync-free torch composition."""
    if mode not in ("histogram", "dominant"):
        raise ValueError(f"mode must be 'histogram' or 'dominant', got {mode!r}")
    return _hist_loss(logits, y_hist, weight, _HL_MODES[mode], -100, confmat)


def histogram_confusion_matrix(pred, target, num_classes, out=None):
    """Confusion matrix [num_classes, num_classes] (int64, ``[true, predicted]``) of segment-level
    predictions against label histograms, as the reference's ``ConfusionMatrix.update``
    (src/metrics/semantic.py:66-107) accumulates it - in exact integers, where the reference sums
    in float32: ``out[t, pred[r]] += target[r, t]`` for ``t < num_classes`` (further columns are
    void).  ``pred``: int labels [rows] or [rows, num_classes] logits / probabilities (first
    maximum).  A 1-D (or [rows, 1]) ``target`` holds labels: those outside [0, num_classes) are
    void.  ``out``: an int64 buffer to ACCUMULATE into (returned); a fresh zero matrix if None."""
    c = int(num_classes)
    if pred.dim() == 2:
        pred = pred.argmax(dim=1)
    pred = pred.long()
    if target.is_floating_point() or target.dim() not in (1, 2) or target.shape[0] != pred.shape[0]:
        raise ValueError("the target must be an integer [rows] or [rows, ncols] tensor matching pred")
    if target.dim() == 2 and target.shape[1] == 1 and c > 1:
        target = target[:, 0]
    if target.dim() == 2 and target.shape[1] < c:
        raise ValueError(f"a label histogram for {c} classes has at least {c} columns, "
                         f"got {tuple(target.shape)}")
    if out is None:
        out = torch.zeros(c, c, dtype=torch.int64, device=pred.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (c, c) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 [{c}, {c}] tensor")
    rows = pred.shape[0]
    if rows == 0:
        return out
    if pred.is_cuda and c <= 32:
        _lib.require_cuda(target, out)
        pr, tg = _dense(pred, torch.int64, 8), _dense(target, torch.int64, 8)
        with torch.cuda.device(pred.device):
            st = _lib.lib.spt_confusion_matrix_i64(
                _lib.ptr(pr), _lib.ptr(tg), rows, c, tg.shape[1] if tg.dim() == 2 else 0,
                _lib.ptr(out), _lib.stream_ptr(pred.device))
        _lib.check(st, "spt_confusion_matrix_i64")
        return out
    ok = (pred >= 0) & (pred < c)
    pc = pred.clamp(0, c - 1)
    if target.dim() == 2:
        out.index_add_(1, pc, (target[:, :c].long() * ok[:, None]).t().contiguous())
    else:
        ok = ok & (target >= 0) & (target < c)
        out.view(-1).index_add_(0, target.long().clamp(0, c - 1) * c + pc, ok.long())
    return out


# ---------------------------------------------------------------------------
# Edge-affinity loss of the panoptic model (csrc/loss.hip): BCE with logits over the edges that do
# not join two void nodes, weighted by the edge's case, and the binary counters of the same pass
# ---------------------------------------------------------------------------
class _EdgeAffinityLossTorch(torch.autograd.Function):
    """The kernels' rules as a torch composition (CPU tensors): fixed output sizes only, the term
    and the gradient in float64 like the kernels, one rounding to the logits' dtype each."""

    @staticmethod
    def forward(ctx, logits, target, edge_index, node_void, node_obj, node_y, cw, pw, stats, status):
        n = node_void.shape[0]
        i, j = edge_index[0], edge_index[1]
        ok = (i >= 0) & (i < n) & (j >= 0) & (j < n)
        ic, jc = i.clamp(0, n - 1), j.clamp(0, n - 1)
        void = node_void.bool()
        keep = ok & ~(void[ic] & void[jc])
        kind = 2 * (node_y[ic] != node_y[jc]).long() + (node_obj[ic] != node_obj[jc]).long()
        w = torch.ones(i.shape[0], dtype=torch.float64, device=logits.device) if cw is None \
            else cw.double()[kind]
        zero = torch.zeros((), dtype=torch.float64, device=logits.device)
        x = torch.where(keep, logits.detach().double(), zero)
        t = target.detach().double()
        pwd = pw.double().reshape(()) if pw is not None else zero + 1
        lw = 1 + (pwd - 1) * t
        l = (1 - t) * x + lw * ((-x).clamp(min=0) + torch.log1p(torch.exp(-x.abs())))
        num = torch.where(keep, w * l, zero).sum()
        den = torch.where(keep, w, zero).sum()
        if stats is not None:
            pred, tgt = logits.detach() > 0, target.detach() > 0.5
            stats += torch.stack([(keep & pred & tgt).sum(), (keep & pred & ~tgt).sum(),
                                  (keep & ~pred & ~tgt).sum(), (keep & ~pred & tgt).sum()])
        if status is not None:
            status[0] += (~ok).sum().to(status.dtype)
        ctx.save_for_backward(x, t, w, keep, lw, pwd, den)
        ctx.meta = logits.dtype
        return (num / den).to(logits.dtype)

    @staticmethod
    def backward(ctx, gout):
        x, t, w, keep, lw, pwd, den = ctx.saved_tensors
        g = gout.detach().double() * w / den * (lw * torch.sigmoid(x) - pwd * t)
        return (torch.where(keep, g, torch.zeros_like(g)).to(ctx.meta),) + (None,) * 9


class _EdgeAffinityLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, edge_index, node_void, node_obj, node_y, cw, pw, stats, status):
        _lib.require_cuda(logits, target, edge_index, node_void, node_obj, node_y, cw, pw, stats,
                          status)
        lg, tg = _f32c(logits), _f32c(target)
        e, n = lg.shape[0], node_void.shape[0]
        dev = lg.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        den = torch.empty(1, dtype=torch.float64, device=dev)
        nbytes = _lib.lib.spt_edge_affinity_loss_workspace_bytes(e)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_edge_affinity_loss_fwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), _lib.ptr(edge_index), e, _lib.ptr(node_void),
                _lib.ptr(node_obj), _lib.ptr(node_y), n, _lib.ptr(cw), _lib.ptr(pw),
                _lib.ptr(loss), _lib.ptr(den), _lib.ptr(stats), _lib.ptr(status), _lib.ptr(ws),
                nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_edge_affinity_loss_fwd_f32")
        ctx.save_for_backward(lg, tg, edge_index, node_void, node_obj, node_y, cw, pw, den)
        ctx.meta = logits.dtype
        return loss[0].to(logits.dtype)

    @staticmethod
    def backward(ctx, gout):
        lg, tg, edge_index, node_void, node_obj, node_y, cw, pw, den = ctx.saved_tensors
        e, n = lg.shape[0], node_void.shape[0]
        dev = lg.device
        g = _dense(gout.detach().reshape(1), torch.float32, 4)
        glog = torch.empty_like(lg)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_edge_affinity_loss_bwd_f32(
                _lib.ptr(lg), _lib.ptr(tg), _lib.ptr(edge_index), e, _lib.ptr(node_void),
                _lib.ptr(node_obj), _lib.ptr(node_y), n, _lib.ptr(cw), _lib.ptr(pw), _lib.ptr(g),
                _lib.ptr(den), _lib.ptr(glog), _lib.stream_ptr(dev))
        _lib.check(st, "spt_edge_affinity_loss_bwd_f32")
        return (glog.to(ctx.meta),) + (None,) * 9


def edge_affinity_loss(logits, target, edge_index, node_void, node_obj, node_y, case_weights=None,
                       pos_weight=None, stats=None, status=None):
    """The edge-affinity loss of ``PanopticSegmentationModule.model_step``
    (src/models/panoptic.py:726-796) without compacting anything: BCE with logits of ``logits``
    f32 ``[E]`` against ``target`` f32 ``[E]`` in [0, 1] over the edges ``edge_index`` int64
    ``[2, E]`` that do not join two void nodes (``node_void`` bool ``[N]``:
    ``predict.void_mask(y_hist)``), differentiable in ``logits``.

    ``node_obj`` / ``node_y`` int64 ``[N]``: the nodes' major object and its label
    (``panoptic.major_objects``).  ``case_weights``: 4 weights for ``[same-class same-obj,
    same-class diff-obj, diff-class same-obj, diff-class diff-obj]`` - the loss is then
    ``sum(w l) / sum(w)`` over the kept edges (``WeightedBCEWithLogitsLoss``); ``None``: their
    mean (``BCEWithLogitsLoss``).  ``pos_weight``: a number or a 1-element tensor (read on the
    device).  A list of weights is copied to the device on every call, which a graph capture
    refuses: inside a captured step pass device tensors (``criterion.EdgeAffinityCriterion``
    keeps both as buffers).  No kept edge gives NaN (the mean of an empty tensor) and an
    all-zero gradient.

    ``stats``: optional int64 ``[4]`` buffer; tp, fp, tn, fn of ``logits > 0`` against
    ``target > 0.5`` over the kept edges are ADDED to it by the same pass.  ``status``: optional
    int32 ``[1]`` buffer counting edges with an end outside ``[0, N)``, which are dropped.
    CUDA tensors run on the HIP kernels with no host synchronisation (the call can be captured
    into a graph) and bitwise reproducibly; CPU tensors take a torch composition of the same
    rules."""
    if logits.dim() != 1 or not logits.is_floating_point():
        raise ValueError(f"logits must be a floating [E] tensor, got {tuple(logits.shape)}")
    e = logits.shape[0]
    if tuple(target.shape) != (e,) or not target.is_floating_point():
        raise ValueError(f"target must be a floating [{e}] tensor, got {tuple(target.shape)}")
    if tuple(edge_index.shape) != (2, e) or edge_index.is_floating_point():
        raise ValueError(f"edge_index must be an integer [2, {e}] tensor, got {tuple(edge_index.shape)}")
    if node_void.dim() != 1 or node_void.dtype not in (torch.bool, torch.uint8):
        raise ValueError("node_void must be a bool or uint8 [N] tensor")
    n = node_void.shape[0]
    if tuple(node_obj.shape) != (n,) or tuple(node_y.shape) != (n,) \
            or node_obj.is_floating_point() or node_y.is_floating_point():
        raise ValueError(f"node_obj and node_y must be integer [{n}] tensors")
    dev = logits.device
    for name, t in (("target", target), ("edge_index", edge_index), ("node_void", node_void),
                    ("node_obj", node_obj), ("node_y", node_y)):
        if t.device != dev:
            raise ValueError(f"{name} lives on {t.device}, the logits on {dev}")
    cw = pw = None
    if case_weights is not None:
        cw = _dense(torch.as_tensor(case_weights, dtype=torch.float32, device=dev))
        if tuple(cw.shape) != (4,):
            raise ValueError(f"case_weights must hold 4 values, got {tuple(cw.shape)}")
    if pos_weight is not None:
        if torch.is_tensor(pos_weight):
            if pos_weight.numel() != 1:
                raise ValueError("pos_weight must be a scalar (one weight for the one output)")
            pw = _dense(pos_weight.detach().to(device=dev, dtype=torch.float32).reshape(1))
        else:
            pw = torch.full((1,), float(pos_weight), dtype=torch.float32, device=dev)
    if stats is not None and (stats.dtype != torch.int64 or tuple(stats.shape) != (4,)
                              or not stats.is_contiguous() or stats.device != dev):
        raise ValueError(f"stats must be a contiguous int64 [4] tensor on {dev}")
    if status is not None and (status.dtype != torch.int32 or status.numel() < 1
                               or not status.is_contiguous() or status.device != dev):
        raise ValueError(f"status must be a contiguous int32 tensor on {dev}")
    if e == 0:                                    # decided from the shape: the mean of nothing
        return logits.sum() + float("nan")
    if n == 0:
        raise ValueError("edges over an empty node set")
    ei = _dense(edge_index.detach(), torch.int64, 8)
    void = _dense(node_void.detach(), None, 1)
    obj, y = _dense(node_obj.detach(), torch.int64, 8), _dense(node_y.detach(), torch.int64, 8)
    if logits.is_cuda:
        return _EdgeAffinityLoss.apply(logits, target.detach(), ei, void, obj, y, cw, pw, stats,
                                       status)
    return _EdgeAffinityLossTorch.apply(logits, target, ei, void, obj, y, cw, pw, stats, status)


# ---------------------------------------------------------------------------
# Edge-contrast focal loss of the partition training stage (csrc/partition_loss.hip): node labels,
# edge classes, the adaptive sample and the loss on the device; the backward walks CSR runs
# ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1
PARTITION_STATUS_CLAMPED = 1      # status[1]: the sample wanted more intra edges than there are


def _rand32_int(seed, i):
    """``rand32`` of csrc/rng.hpp in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z = z ^ (z >> 31)
    return z >> 32


def partition_call_seed(seed, calls):
    """The stream of call number ``calls`` of a ``(seed, calls)`` state (``pl_call_seed``)."""
    mask = (_rand32_int(0x5EED, 2 * calls) << 32) | _rand32_int(0x5EED, 2 * calls + 1)
    return ((seed & _M64) ^ mask) & _M64


def _i64c(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _rand32_torch(seed, n, device):
    """``rand32(seed, 0 .. n - 1)`` as int64 values in [0, 2**32): int64 products wrap like the
    kernels' uint64 ones, the logical shifts are masked arithmetic ones."""
    def lsr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)
    i = torch.arange(1, n + 1, dtype=torch.int64, device=device)
    z = i * _i64c(0x9E3779B97F4A7C15) + _i64c(seed)
    z = (z ^ lsr(z, 30)) * _i64c(0xBF58476D1CE4E5B9)
    z = (z ^ lsr(z, 27)) * _i64c(0x94D049BB133111EB)
    z = z ^ lsr(z, 31)
    return lsr(z, 32)


def _partition_edge_loss_torch(x, y, ei, c, temperature, gamma, weight, epsilon, ratio, state,
                               counts, status, selected):
    """The kernels' rules as a torch composition (CPU tensors): the same decisions and the same
    sample; the terms in float64 under autograd, whose ``norm`` backward is 0 at distance 0."""
    n, e = x.shape[0], ei.shape[1]
    if y.dim() == 1:
        label = torch.where((y >= 0) & (y < c), y.long(), torch.full_like(y.long(), -1))
    else:
        best, label = y[:, :c].long().max(dim=1)
        first = (y[:, :c].long() == best[:, None]).int().argmax(dim=1)   # ties to the lowest label
        label = torch.where(best == 0, torch.full_like(first, -1), first)
    i, j = ei[0], ei[1]
    ok = (i >= 0) & (i < n) & (j >= 0) & (j < n)
    ic, jc = i.clamp(0, n - 1), j.clamp(0, n - 1)
    kept = ok & (i != j) & (label[ic] >= 0) & (label[jc] >= 0)
    intra = kept & (label[ic] == label[jc])
    inter = kept & ~intra
    n_inter, n_intra = int(inter.sum()), int(intra.sum())
    clamped = 0
    sel = kept
    if ratio is not None:
        fr = torch.tensor(1.0 / ratio - 1.0, dtype=torch.float32)
        n_major = int((torch.tensor(n_inter, dtype=torch.float32) * fr).long())
        if n_major > n_intra:
            n_major, clamped = n_intra, 1
        n_major = max(n_major, 0)
        seed = partition_call_seed(int(state[0]), int(state[1]))
        draw = _rand32_torch(seed, e, ei.device)
        draw = torch.where(intra, draw, torch.full_like(draw, 1 << 40))
        order = torch.sort(draw, stable=True).indices[:n_major]      # ties to the lower position
        sel = inter.clone()
        sel[order] = True
        state[1] += 1
    else:
        n_major = n_intra
    n_sel = n_inter + n_major
    if counts is not None:
        counts.copy_(torch.tensor([n_inter, n_intra, n_sel], dtype=torch.int64))
    if status is not None:
        status[0] += int((~ok).sum())
        status[1] |= clamped
    if selected is not None:
        selected.copy_(sel.to(selected.dtype))
    if n_inter == 0 or n_sel == 0:
        return (x * 0).sum()                       # exactly 0, an all-zero gradient
    idx = sel.nonzero()[:, 0]
    t = intra[idx]
    xd = x.double()
    d = (xd[i[idx]] - xd[j[idx]]).norm(dim=1)
    p = torch.exp(-d / temperature)
    q = torch.where(t, p, 1 - p)
    qp = epsilon + (1 - 2 * epsilon) * q
    w = torch.where(t, torch.full_like(qp, weight), torch.full_like(qp, 1 - weight))
    mod = torch.ones_like(qp) if gamma == 0 else (1 - qp) ** gamma
    return ((-w * mod * torch.log(qp)).sum() / n_sel).to(x.dtype)


class _PartitionEdgeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, ei, holder, c, params, ratio, state, counts, status, selected):
        xs = x.detach()
        if xs.dtype != torch.float32:
            xs = xs.float()
        n, d = xs.shape
        if xs.stride(1) != 1 or (n > 1 and xs.stride(0) < d) or xs.data_ptr() % 4:
            xs = xs.contiguous()
        ldx = xs.stride(0) if n > 1 else d
        e = ei.shape[1]
        dev = xs.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        den = torch.empty(1, dtype=torch.float64, device=dev)
        code = torch.empty(e, dtype=torch.uint8, device=dev)
        nbytes = _lib.lib.spt_partition_loss_workspace_bytes(n, e)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_partition_loss_fwd_f32(
                _lib.ptr(xs), ldx, n, d, _lib.ptr(y), y.shape[1] if y.dim() == 2 else 0, c,
                _lib.ptr(ei), e, *params, -1.0 if ratio is None else float(ratio), _lib.ptr(state),
                _lib.ptr(loss), _lib.ptr(den), _lib.ptr(code), _lib.ptr(counts), _lib.ptr(status),
                _lib.ptr(selected), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_partition_loss_fwd_f32")
        ctx.save_for_backward(xs, ei, code, den)
        ctx.meta = (x.dtype, ldx, params, holder)
        return loss[0].to(x.dtype)

    @staticmethod
    def backward(ctx, gout):
        from .csr import edge_end_views
        xs, ei, code, den = ctx.saved_tensors
        dtype, ldx, params, holder = ctx.meta
        n, d = xs.shape
        e = ei.shape[1]
        dev = xs.device
        by_src, by_tgt = edge_end_views(holder[0], n)     # memoised on the caller's edge_index
        g = _dense(gout.detach().reshape(1), torch.float32, 4)
        gx = torch.empty((n, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_partition_loss_bwd_f32(
                _lib.ptr(xs), ldx, n, d, _lib.ptr(ei), e, _lib.ptr(code), _lib.ptr(by_src.rowptr),
                _lib.ptr(by_src.perm), _lib.ptr(by_tgt.rowptr), _lib.ptr(by_tgt.perm), *params,
                _lib.ptr(g), _lib.ptr(den), _lib.ptr(gx), d, _lib.stream_ptr(dev))
        _lib.check(st, "spt_partition_loss_bwd_f32")
        return (gx.to(dtype),) + (None,) * 10


def partition_edge_loss(x, y, edge_index, num_classes, temperature=1, gamma=0, weight=0.5,
                        epsilon=1e-6, ratio=None, state=None, counts=None, status=None,
                        selected=None):
    """The loss of the partition training stage (``PartitionCriterion.edge_classification_loss``
    with ``BinaryFocalLoss``, src/loss/partition_criterion.py:92-145, src/loss/focal.py:194-220),
    differentiable in ``x`` f32 ``[N, D]`` (``D <= 128``; any row stride).

    ``y``: int label histograms ``[N, num_classes + 1]`` (the node's label is the first maximum of
    the class columns; a node whose maximum is 0 is void) or an int label vector ``[N]`` with
    ``num_classes`` (or anything outside ``[0, num_classes)``) for void.  ``edge_index`` int
    ``[2, E]`` in any order.  Self loops and edges with a void end are dropped; the others are
    intra (same label, target affinity 1) or inter (0).  Per selected edge the affinity
    ``exp(-|x_i - x_j| / temperature)`` enters the binary focal loss (``gamma``, ``weight`` of the
    intra class, ``epsilon``); the result is the mean over the selected edges, exactly 0 (with an
    all-zero gradient) when nothing is selected or there is no inter edge.

    ``ratio`` (``adaptive_sampling_ratio``; None: every kept edge is selected): all inter edges
    and ``int(f32(n_inter) * f32(1 / ratio - 1))`` intra edges, drawn on the device from
    ``state``, an int64 ``[2]`` tensor ``(seed, calls)`` on ``x``'s device whose second entry the
    call advances: the same state gives the same sample, a replayed graph draws a fresh one each
    time.  Without a ``state`` the call draws from ``(0, 0)``.

    ``counts``: optional int64 ``[3]`` buffer, WRITTEN with ``n_inter, n_intra, n_selected``.
    ``status``: optional int32 ``[2]`` buffer; ``[0] +=`` the edges with an end outside
    ``[0, N)`` (dropped), ``[1] |= PARTITION_STATUS_CLAMPED`` where the reference would have
    asserted (fewer intra edges than the sample asks for: all are taken).  ``selected``: optional
    uint8 ``[E]`` output, 1 for a selected edge.

    CUDA tensors run on the HIP kernels with no host synchronisation (the call can be captured
    into a graph) and bitwise reproducibly - the backward sums per node over the by-source and
    by-target views of ``edge_index`` (``csr.edge_end_views``, sorted once per edge list) instead
    of scattering with atomics; CPU tensors take a torch composition of the same rules."""
    if x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"x must be a floating [N, D] tensor, got {tuple(x.shape)}")
    n, d = x.shape
    if d < 1 or d > 128:
        raise ValueError(f"rows of 1 to 128 features are supported, got {d}")
    c = int(num_classes)
    if c < 1:
        raise ValueError("num_classes must be positive")
    if y.is_floating_point() or y.dtype == torch.bool or y.dim() not in (1, 2) or y.shape[0] != n \
            or (y.dim() == 2 and y.shape[1] < c):
        raise ValueError(f"y must be an integer [{n}] label vector or [{n}, >= {c}] histogram, "
                         f"got {tuple(y.shape)} {y.dtype}")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.is_floating_point():
        raise ValueError(f"edge_index must be an integer [2, E] tensor, got {tuple(edge_index.shape)}")
    e = edge_index.shape[1]
    temperature, gamma, weight, epsilon = (float(temperature), float(gamma), float(weight),
                                           float(epsilon))
    if not temperature > 0 or not gamma >= 0 or not 0 <= weight <= 1 or not 0 <= epsilon < 0.5:
        raise ValueError("temperature > 0, gamma >= 0, weight in [0, 1] and epsilon in [0, 0.5) "
                         f"are needed, got {temperature}, {gamma}, {weight}, {epsilon}")
    if ratio is not None and not 0 < float(ratio) <= 1:
        raise ValueError(f"ratio must lie in (0, 1] or be None, got {ratio}")
    dev = x.device
    for name, t in (("y", y), ("edge_index", edge_index), ("state", state), ("counts", counts),
                    ("status", status), ("selected", selected)):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} lives on {t.device}, x on {dev}")
    if state is not None and (state.dtype != torch.int64 or tuple(state.shape) != (2,)
                              or not state.is_contiguous()):
        raise ValueError("state must be a contiguous int64 [2] tensor (seed, calls)")
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (3,)
                               or not counts.is_contiguous()):
        raise ValueError("counts must be a contiguous int64 [3] tensor")
    if status is not None and (status.dtype != torch.int32 or tuple(status.shape) != (2,)
                               or not status.is_contiguous()):
        raise ValueError("status must be a contiguous int32 [2] tensor")
    if selected is not None and (selected.dtype != torch.uint8 or tuple(selected.shape) != (e,)
                                 or not selected.is_contiguous()):
        raise ValueError(f"selected must be a contiguous uint8 [{e}] tensor")
    if e == 0:
        raise ValueError("No edges found in batch.")
    if n >= 1 << 31 or e >= 1 << 31:
        raise ValueError("more than 2^31 - 1 nodes or edges")
    if ratio is not None and state is None:
        state = torch.zeros(2, dtype=torch.int64, device=dev)
    if ratio is None:
        state = None
    ratio = None if ratio is None else float(ratio)
    if not x.is_cuda:
        return _partition_edge_loss_torch(x, y.detach(), edge_index.detach().long(), c, temperature,
                                          gamma, weight, epsilon, ratio, state, counts, status,
                                          selected)
    ei = _dense(edge_index.detach(), torch.int64, 8)
    yd = _dense(y.detach(), torch.int64, 8)
    return _PartitionEdgeLoss.apply(x, yd, ei, (edge_index,), c, (temperature, gamma, weight, epsilon),
                                    ratio, state, counts, status, selected)


# ---------------------------------------------------------------------------
# Fused MLP: [bias-free Linear -> GraphNorm -> LeakyReLU] x L  (src/nn/mlp.py:8-94)
# ---------------------------------------------------------------------------
_GPTR_ATTR = "_spt_graph_ranges"


def _host_ptr(batch, num_graphs):
    """Row ranges [B+1] of the clouds of a batch vector when its maker left them on the tensor
    (``NAG.from_nag_list`` / the synthetic batches: ``Batch.ptr`` of the reference) - host
    knowledge, no device read-back - else None."""
    hp = getattr(batch, "_spt_host_ptr", None)
    if (hp is None or len(hp) != int(num_graphs) + 1 or hp[0] != 0 or hp[-1] != batch.numel()
            or batch._version != 0):
        return None
    return list(hp)


def graph_ranges(batch, num_graphs, rows):
    """Host row ranges [B+1] of the graphs when ``batch`` is sorted (clouds of a
    NAGBatch are contiguous), else None.  One host sync per batch tensor (memoised
    on the tensor, like the CSR views)."""
    if batch is None or (num_graphs is not None and int(num_graphs) == 1):
        return [0, rows]                                 # one graph: nothing to look at
    memo = getattr(batch, _GPTR_ATTR, None)
    key = (batch._version, int(num_graphs), batch.data_ptr(), batch.numel())
    if memo is not None and memo[0] == key:
        return memo[1]
    hp = _host_ptr(batch, num_graphs)
    if hp is not None:
        return hp
    if batch.numel() and not bool((batch[1:] >= batch[:-1]).all()):
        ranges = None
    else:
        counts = torch.bincount(batch, minlength=int(num_graphs)).tolist()
        ranges = [0]
        for c_ in counts:
            ranges.append(ranges[-1] + c_)
    try:
        setattr(batch, _GPTR_ATTR, (key, ranges))
    except Exception:
        pass
    return ranges


MAX_FUSED_RUNS = 16          # FMLP_MAX_RUNS of csrc/common.hpp


class GraphRuns:
    """Row ranges of constant graph id, sorted by graph: what one launch of the fused layer
    kernels covers (``spt_fused_linear_*_runs_f32``).  ``sorted_batch``: one run per graph in
    row order (a batch whose clouds are contiguous)."""

    __slots__ = ("r0", "r1", "g", "B", "rows", "sorted_batch", "_c")

    def __init__(self, runs, B, rows):
        runs = sorted(runs, key=lambda t: (t[2], t[0]))
        self.r0 = [int(t[0]) for t in runs]
        self.r1 = [int(t[1]) for t in runs]
        self.g = [int(t[2]) for t in runs]
        self.B, self.rows = int(B), int(rows)
        self.sorted_batch = (len(runs) <= self.B and
                             all(self.r1[i] <= self.r0[i + 1] for i in range(len(runs) - 1)))
        self._c = None

    @property
    def n(self):
        return len(self.r0)

    def c_arrays(self):
        """(nruns, int64[] r0, int64[] r1, int32[] graph) for the C ABI (host arrays)."""
        if self._c is None:
            import ctypes
            n = self.n
            self._c = (n, (ctypes.c_int64 * n)(*self.r0), (ctypes.c_int64 * n)(*self.r1),
                       (ctypes.c_int32 * n)(*self.g))
        return self._c

    def rows_per_graph(self):
        out = [0] * self.B
        for a, b, g in zip(self.r0, self.r1, self.g):
            out[g] += b - a
        return out


def graph_runs(batch, num_graphs, rows):
    """``GraphRuns`` of a per-row graph index, or None when it has more than 16 runs / graphs
    (the caller then takes the layer-by-layer route).  ``batch`` may be sorted (one run per
    cloud) or piecewise sorted (the edge MLP's norm index).  One host sync per batch tensor
    (memoised on the tensor, like the CSR views)."""
    if batch is None or (num_graphs is not None and int(num_graphs) == 1):
        return GraphRuns([(0, rows, 0)], 1, rows)
    B = int(num_graphs)
    if B > MAX_FUSED_RUNS:
        return None
    memo = getattr(batch, _GRUN_ATTR, None)
    key = (batch._version, B, batch.data_ptr(), batch.numel())
    if memo is not None and memo[0] == key:
        return memo[1]
    runs = None
    hp = _host_ptr(batch, B)
    if batch.numel() == 0:
        runs = GraphRuns([], B, 0)
    elif hp is not None:
        runs = GraphRuns([(hp[g], hp[g + 1], g) for g in range(B) if hp[g + 1] > hp[g]], B,
                         batch.numel())
    else:
        # run starts = positions where the id changes; read back only when there are few
        change = (batch[1:] != batch[:-1])
        n_change = int(change.sum())
        if n_change + 1 <= MAX_FUSED_RUNS:
            starts = [0] + (torch.nonzero(change).flatten() + 1).tolist()
            ends = starts[1:] + [int(batch.numel())]
            ids = batch[torch.tensor(starts, device=batch.device)].tolist()
            if all(0 <= g < B for g in ids):
                runs = GraphRuns(list(zip(starts, ends, ids)), B, batch.numel())
    try:
        setattr(batch, _GRUN_ATTR, (key, runs))
    except Exception:
        pass
    return runs


_GRUN_ATTR = "_spt_graph_runs"


def graph_runs_via(batch, num_graphs, holder, *deps):
    """``graph_runs(batch, ...)`` for a ``batch`` that is DERIVED from longer-lived tensors (the
    edge MLP's ``norm_index[edge_index[0]]`` is rebuilt every forward): the run table - host
    knowledge of the batch layout, like the row ranges of ``batch`` itself - is memoised on
    ``holder`` (the edge_index) keyed by the versions of ``deps``, so only the first forward on a
    batch pays the read-back."""
    key = tuple((d._version, d.data_ptr(), d.numel()) for d in deps) + (int(num_graphs),)
    memo = getattr(holder, _GRUN_ATTR + "_via", None)
    host = getattr(holder, "_spt_host_runs", None)
    if memo is not None and memo[0] == key:
        runs = memo[1]
    elif (host is not None and holder._version == 0 and host[0] == (int(num_graphs), batch.numel())
          and len(host[1]) <= MAX_FUSED_RUNS):
        # the batch's maker left the runs on the edge index (host knowledge of the batch layout,
        # like Batch.ptr: per-cloud edge counts are known where the clouds are concatenated)
        runs = GraphRuns(list(host[1]), int(num_graphs), batch.numel())
    else:
        runs = graph_runs(batch, num_graphs, batch.numel())
        try:
            setattr(holder, _GRUN_ATTR + "_via", (key, runs))
        except Exception:
            pass
    try:
        setattr(batch, _GRUN_ATTR, ((batch._version, int(num_graphs), batch.data_ptr(), batch.numel()), runs))
    except Exception:
        pass
    return runs


def fused_mlp_supported(dims):
    return all(_lib.lib.spt_fused_linear_supported(int(k), int(n))
               for k, n in zip(dims[:-1], dims[1:]))


_ST_H, _ST_X = 8, 16          # SPT_FMLP_H_BF16 / SPT_FMLP_X_BF16 of include/spt_hip.h


def _fmlp_forward(x, batch, runs, eps_list, slope_list, params, apply_last=True, fmode=-1,
                  store16=False):
    """Forward of the fused layer chain (``runs``: a ``GraphRuns``; ONE launch per layer whatever
    the number of graphs).  Returns (y or None, saved tensors, hs[-1], tables of
    the last GraphNorm): with ``apply_last=False`` the last norm + activation are left to the
    consumer (the fused max-pool)."""
    L = len(eps_list)
    Ws = [_dense(params[4 * i].detach(), torch.float32) for i in range(L)]
    gnw = [_dense(params[4 * i + 1].detach(), torch.float32) for i in range(L)]
    gnb = [_dense(params[4 * i + 2].detach(), torch.float32) for i in range(L)]
    gms = [_dense(params[4 * i + 3].detach(), torch.float32) for i in range(L)]
    x2 = _dense(x.detach(), torch.float32)
    batch = _dense(batch, torch.int64, 8)        # (the run table came from the caller's tensor)
    R = x2.shape[0]
    dev = x2.device
    B = runs.B
    nr, c_r0, c_r1, c_g = runs.c_arrays()
    sp = _lib.stream_ptr(dev)
    hs, tabs = [], []
    cur, pre = x2, None
    y = None
    with torch.cuda.device(dev):
        for l in range(L):
            N, K = Ws[l].shape
            # store16: raw layer outputs kept as bf16 (bf16 matrix mode: 3), read as bf16 by the
            # next layer (its x), the pool and the backward
            h = torch.empty((R, N), dtype=torch.bfloat16 if store16 else torch.float32, device=dev)
            lmode = (3 | _ST_H | (_ST_X if l else 0)) if store16 else fmode
            total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
            nb = _lib.lib.spt_fused_linear_workspace_bytes(K, N)
            ws = _workspace(nb, dev)
            pa = ps = pb = None
            if pre is not None:
                pa, ps, pb = pre
            mean = torch.empty((B, N), dtype=torch.float32, device=dev)
            rstd, am, sc = (torch.empty_like(mean) for _ in range(3))
            if FUSE_POST:
                # the layer's totals AND its norm's tables out of one post launch
                norm = _lib.GnFwdTables(_lib.ptr(gnw[l]), _lib.ptr(gms[l]), float(eps_list[l]),
                                        _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(am), _lib.ptr(sc))
                with _timed(f"fused_linear_fwd:{K}x{N}:{R}"):
                    st = _lib.lib.spt_fused_linear_fwd_runs_gn_f32(
                        _lib.ptr(cur), nr, c_r0, c_r1, c_g, B, K, _lib.ptr(Ws[l]), N,
                        _lib.ptr(pa), _lib.ptr(ps), _lib.ptr(pb),
                        float(slope_list[l - 1]) if l else 1.0, _lib.ptr(h),
                        _lib.ptr(total), lmode, _lib.ptr(ws), ws.numel(), ctypes.addressof(norm), sp)
                _lib.check(st, "spt_fused_linear_fwd_runs_gn_f32")
            else:
                with _timed(f"fused_linear_fwd:{K}x{N}:{R}"):
                    st = _lib.lib.spt_fused_linear_fwd_runs_f32(
                        _lib.ptr(cur), nr, c_r0, c_r1, c_g, B, K, _lib.ptr(Ws[l]), N,
                        _lib.ptr(pa), _lib.ptr(ps), _lib.ptr(pb),
                        float(slope_list[l - 1]) if l else 1.0, _lib.ptr(h),
                        _lib.ptr(total), lmode, _lib.ptr(ws), ws.numel(), sp)
                _lib.check(st, "spt_fused_linear_fwd_runs_f32")
                st = _lib.lib.spt_graphnorm_tables_f32(
                    _lib.ptr(total), B, N, _lib.ptr(gnw[l]), _lib.ptr(gms[l]), float(eps_list[l]),
                    _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(am), _lib.ptr(sc), sp)
                _lib.check(st, "spt_graphnorm_tables_f32")
            hs.append(h)
            tabs.append((mean, rstd, am, sc))
            cur, pre = h, (am, sc, gnb[l])
        if apply_last:
            assert not store16, "bf16 storage: the last norm is applied by the consumer (the pool)"
            N = Ws[-1].shape[0]
            y = torch.empty((R, N), dtype=torch.float32, device=dev)
            st = _lib.lib.spt_graphnorm_apply_f32(
                _lib.ptr(hs[-1]), _lib.ptr(batch) if B > 1 else None, R, N, B,
                _lib.ptr(tabs[-1][2]), _lib.ptr(tabs[-1][3]), _lib.ptr(gnb[-1]),
                float(slope_list[-1]), _lib.ptr(y), sp)
            _lib.check(st, "spt_graphnorm_apply_f32")
    saved = (x2, batch, *hs, *[t for tab in tabs for t in tab], *Ws, *gnw, *gnb, *gms)
    return y, saved, hs[-1], (tabs[-1][2], tabs[-1][3], gnb[-1])


# Round 6: a fused layer's table sums and the GraphNorm table kernel that consumes them as ONE post
# launch (spt_fused_linear_*_gn_f32: 2 launches per layer and direction instead of 3 / 4; the same
# sums in the same order, the same formulas - tests pin the two routes on each other bitwise).
FUSE_POST = os.environ.get("SPT_FUSE_POST", "1") != "0"


def fuse_post(on=None):
    global FUSE_POST
    old = FUSE_POST
    if on is not None:
        FUSE_POST = bool(on)
    return old


# The chain's bottom layer folded into the backward of the layer above it: where the
# chain's input needs no gradient, the bottom layer's backward only forms gW0 - from sums the upper
# layer's kernel can take while it holds g' and the tile (spt_fused_linear_bwd_runs_gn_fold_f32): no
# [rows, K] gradient is written or read, no bottom-layer launch.  Default on; SPT_FMLP_FOLD_BOTTOM=0
# or fold_bottom(False) select the layer-by-layer route (A/B, tests).
FOLD_BOTTOM = os.environ.get("SPT_FMLP_FOLD_BOTTOM", "1") != "0"


def fold_bottom(on=None):
    global FOLD_BOTTOM
    old = FOLD_BOTTOM
    if on is not None:
        FOLD_BOTTOM = bool(on)
    return old


def _fmlp_backward(saved, meta, gy, top_total=None, pooled=None, top_tabs=None):
    """Backward of the fused layer chain from the gradient of its (normalised) output.
    ``top_total``: statistics of the top GraphNorm's backward when the caller already has
    them (the max-pool route computes them from the pool's sparse gradient).
    ``pooled = (gout, arg, csr)``: the top layer consumes the pool's gradient directly
    (``spt_fused_linear_bwd_pooled_runs_f32``), ``gy`` is then None."""
    L, runs, slopes, in_dtype, need_gx0 = meta[:5]
    fmode = meta[5] if len(meta) > 5 else -1          # the matrix mode the forward ran in
    store16 = bool(meta[6]) if len(meta) > 6 else False   # layer outputs stored as bf16
    sv = list(saved)
    x2, batch = sv[0], sv[1]
    hs = sv[2:2 + L]
    tabs = [tuple(sv[2 + L + 4 * i: 2 + L + 4 * i + 4]) for i in range(L)]
    o = 2 + 5 * L
    Ws, gnw, gnb, gms = sv[o:o + L], sv[o + L:o + 2 * L], sv[o + 2 * L:o + 3 * L], sv[o + 3 * L:o + 4 * L]
    R = x2.shape[0]
    dev = x2.device
    B = runs.B
    nr, c_r0, c_r1, c_g = runs.c_arrays()
    sp = _lib.stream_ptr(dev)
    g_cur = _dense(gy, torch.float32)
    grads = [None] * (4 * L)
    gx0 = None
    with torch.cuda.device(dev):
        # statistics of the top GraphNorm's backward need their own pass over (h_L, gy)
        N = Ws[-1].shape[0]
        mean, rstd, am, sc = tabs[-1]
        if top_tabs is not None:
            total = None                 # the caller's post launch already wrote the top norm's tables
        elif top_total is not None:
            total = top_total
        else:
            assert not store16, "bf16 storage: the top statistics come from the sparse route"
            total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
            ws = _workspace(_lib.lib.spt_graphnorm_workspace_bytes(R, N, B), dev)
            st = _lib.lib.spt_graphnorm_bwd_stats_f32(
                _lib.ptr(hs[-1]), _lib.ptr(g_cur), _lib.ptr(batch) if B > 1 else None, R, N, B,
                _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb[-1]), float(slopes[-1]), _lib.ptr(total),
                _lib.ptr(ws), ws.numel(), sp)
            _lib.check(st, "spt_graphnorm_bwd_stats_f32")
        cur_tabs = top_tabs
        for l in range(L - 1, -1, -1):
            N, K = Ws[l].shape
            mean, rstd, am, sc = tabs[l]
            if cur_tabs is not None:
                c1, c2, c3, gw_n, gb_n, ga_n = cur_tabs
            else:
                c1, c2, c3 = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(3))
                gw_n, gb_n, ga_n = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
                st = _lib.lib.spt_graphnorm_bwd_tables_f32(
                    _lib.ptr(total), B, N, _lib.ptr(gnw[l]), _lib.ptr(gms[l]), _lib.ptr(mean),
                    _lib.ptr(rstd), _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(gw_n),
                    _lib.ptr(gb_n), _lib.ptr(ga_n), sp)
                _lib.check(st, "spt_graphnorm_bwd_tables_f32")
            xprev = hs[l - 1] if l else x2
            pre = tabs[l - 1] if l else None
            lmode = (3 | _ST_H | (_ST_X if l else 0)) if store16 else fmode
            # the bottom layer rides along (see FOLD_BOTTOM): this layer's gx is then never formed
            fold = (l == 1 and FOLD_BOTTOM and FUSE_POST and not need_gx0 and not store16
                    and not (pooled is not None and l == L - 1)
                    and x2.dtype == torch.float32
                    and bool(_lib.lib.spt_fused_linear_bwd_fold_supported(
                        int(Ws[0].shape[1]), K, N, lmode)))
            want_gx = (l > 0 or need_gx0) and not fold
            gx = torch.empty((R, K), dtype=torch.float32, device=dev) if want_gx else None
            gW = torch.empty((N, K), dtype=torch.float32, device=dev)
            # the previous layer's backward tables: written by THIS call's post launch (FUSE_POST),
            # or by the next iteration's table call from the totals this call leaves
            nxt_tabs, pn = None, None
            if l and FUSE_POST:
                nxt_tabs = (*(torch.empty((B, K), dtype=torch.float32, device=dev) for _ in range(3)),
                            *(torch.empty(K, dtype=torch.float32, device=dev) for _ in range(3)))
                pn = _lib.GnBwdTables(_lib.ptr(gnw[l - 1]), _lib.ptr(gms[l - 1]), _lib.ptr(tabs[l - 1][0]),
                                      _lib.ptr(tabs[l - 1][1]), *[_lib.ptr(t) for t in nxt_tabs])
            ptot = (torch.empty((B, 2 * K + 1), dtype=torch.float64, device=dev)
                    if (l and pn is None) else None)
            ws = _workspace(_lib.lib.spt_fused_linear_workspace_bytes(K, N), dev)
            pa = ps = pb = None
            if pre is not None:
                pa, ps, pb = pre[2], pre[3], gnb[l - 1]
            if fold:
                K0 = int(Ws[0].shape[1])
                gW0 = torch.empty((K, K0), dtype=torch.float32, device=dev)
                with _timed(f"fused_linear_bwd_fold:{K0}x{K}x{N}:{R}"):
                    st = _lib.lib.spt_fused_linear_bwd_runs_gn_fold_f32(
                        _lib.ptr(g_cur), _lib.ptr(hs[l]), nr, c_r0, c_r1, c_g, B, N,
                        _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb[l]), float(slopes[l]),
                        _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(xprev), K,
                        _lib.ptr(pa), _lib.ptr(ps), _lib.ptr(pb), float(slopes[0]), _lib.ptr(Ws[l]),
                        _lib.ptr(gW), lmode, _lib.ptr(ws), ws.numel(), ctypes.addressof(pn),
                        _lib.ptr(x2), K0, _lib.ptr(Ws[0]), _lib.ptr(gW0), sp)
                _lib.check(st, "spt_fused_linear_bwd_runs_gn_fold_f32")
                grads[4], grads[5], grads[6], grads[7] = gW, gw_n, gb_n, ga_n
                grads[0], grads[1], grads[2], grads[3] = gW0, nxt_tabs[3], nxt_tabs[4], nxt_tabs[5]
                break
            if pooled is not None and l == L - 1:
                p_gout, p_arg, p_csr = pooled
                args = (_lib.ptr(p_gout), _lib.ptr(p_arg), _lib.ptr(p_csr.perm),
                        _lib.ptr(p_csr.pos_seg()), _lib.ptr(hs[l]), nr, c_r0, c_r1, c_g, B, N,
                        _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb[l]), float(slopes[l]),
                        _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(xprev), K,
                        _lib.ptr(pa), _lib.ptr(ps), _lib.ptr(pb),
                        float(slopes[l - 1]) if l else 1.0, _lib.ptr(Ws[l]), _lib.ptr(gx),
                        _lib.ptr(gW), _lib.ptr(ptot), lmode, _lib.ptr(ws), ws.numel())
                with _timed(f"fused_linear_bwd_pooled:{K}x{N}:{R}"):
                    if pn is not None:
                        st = _lib.lib.spt_fused_linear_bwd_pooled_runs_gn_f32(*args, ctypes.addressof(pn), sp)
                    else:
                        st = _lib.lib.spt_fused_linear_bwd_pooled_runs_f32(*args, sp)
                _lib.check(st, "spt_fused_linear_bwd_pooled_runs_f32")
            else:
                args = (_lib.ptr(g_cur), _lib.ptr(hs[l]), nr, c_r0, c_r1, c_g, B, N,
                        _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb[l]), float(slopes[l]),
                        _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(xprev), K,
                        _lib.ptr(pa), _lib.ptr(ps), _lib.ptr(pb),
                        float(slopes[l - 1]) if l else 1.0, _lib.ptr(Ws[l]), _lib.ptr(gx),
                        _lib.ptr(gW), _lib.ptr(ptot), lmode, _lib.ptr(ws), ws.numel())
                if pn is not None:
                    st = _lib.lib.spt_fused_linear_bwd_runs_gn_f32(*args, ctypes.addressof(pn), sp)
                else:
                    st = _lib.lib.spt_fused_linear_bwd_runs_f32(*args, sp)
                _lib.check(st, "spt_fused_linear_bwd_runs_f32")
            grads[4 * l], grads[4 * l + 1], grads[4 * l + 2], grads[4 * l + 3] = gW, gw_n, gb_n, ga_n
            if l:
                g_cur, total, cur_tabs = gx, ptot, nxt_tabs
            else:
                gx0 = gx
    return (None if gx0 is None else gx0.to(in_dtype)), grads


class _FusedMLP(torch.autograd.Function):
    """All layers of one MLP in one autograd node: raw layer outputs h_l are the
    only [rows, C] tensors kept; normalised activations are never materialised
    except the final output."""

    @staticmethod
    def forward(ctx, x, batch, runs, eps_list, slope_list, *params):
        fmode = _precision.fused_mode()
        y, saved, _, _ = _fmlp_forward(x, batch, runs, eps_list, slope_list, params, fmode=fmode)
        ctx.save_for_backward(*saved)
        ctx.meta = (len(eps_list), runs, list(slope_list), x.dtype, x.requires_grad, fmode)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        gx0, grads = _fmlp_backward(ctx.saved_tensors, ctx.meta, gy)
        return (gx0, None, None, None, None, *grads)


# the fused MLP + max-pool node lets the pool write the winners' raw values for its backward
# (tests switch it off to pin the two routes on each other)
POOL_RAW_OUTPUT = True

# Round 5: the top layer and the max-pool behind it as ONE algebraic unit (csrc/fused_pool.hip) -
# the layer's [rows, N] output is never written, read or recomputed: the forward pools the raw
# tile out of the matrix-pipe accumulators, the norm's statistics come from the Gram matrix of the
# layer's input, the backward needs (gout, arg, raw) and that input only.  Off: the round-4 route
# (layer output materialised, streaming segment-max, LDS-DMA backward); tests pin one on the other.
POOL_IN_FORWARD = os.environ.get("SPT_POOL_IN_FORWARD", "1") != "0"


def pool_in_forward(on=None):
    """Switch of the pool-fused top layer (default on; ``SPT_POOL_IN_FORWARD=0`` turns it off).
    Returns the previous setting."""
    global POOL_IN_FORWARD
    prev = POOL_IN_FORWARD
    if on is not None:
        POOL_IN_FORWARD = bool(on)
    return prev


class _FusedMLPMaxPool(torch.autograd.Function):
    """The fused MLP followed by a max-pool over segments, as ONE node: the last
    GraphNorm-apply + LeakyReLU run inside the pool's read of the raw h_L (the normalised
    [rows, C] tensor is never written).  Backward = the pool's scatter of the incoming
    gradient to the arg rows, then the MLP backward."""

    @staticmethod
    def forward(ctx, x, batch, runs, eps_list, slope_list, csr, seg_graph, *params):
        fmode = _precision.fused_mode()
        # bf16 mode: the raw layer outputs are STORED as bf16 where every kernel of the chain is
        # built for it (the point MLP in front of the L0 -> L1 pool)
        L = len(eps_list)
        dims = [params[0].shape[1]] + [params[4 * i].shape[0] for i in range(L)]
        store16 = bool(
            _precision.bf16_activation_storage()
            and all(_lib.lib.spt_fused_linear_storage_supported(int(k), int(n))
                    for k, n in zip(dims[:-1], dims[1:]))
            and all(int(k) % 32 == 0 for k in dims[1:-1])
            and 256 % int(dims[-1]) == 0
            and _lib.lib.spt_segcsr_max_affine_bf16_supported(int(dims[-1]), x.shape[0]))
        ctx.pool_fused = False
        mode_top = (3 | _ST_X) if store16 else fmode
        if (POOL_IN_FORWARD and L > 1 and runs.sorted_batch
                and _lib.lib.spt_fused_linear_pool_supported(int(dims[-2]), int(dims[-1]), mode_top)
                and (runs.B == 1 or graph_ranges(seg_graph, runs.B, csr.num_seg) is not None)):
            return _FusedMLPMaxPool._forward_pooled(ctx, x, batch, runs, eps_list, slope_list, csr,
                                                    seg_graph, params, fmode, store16, mode_top)
        _, saved, h_last, (am, sc, bs) = _fmlp_forward(x, batch, runs, eps_list, slope_list,
                                                        params, apply_last=False, fmode=fmode,
                                                        store16=store16)
        R, N = h_last.shape
        dev = h_last.device
        out = torch.empty((csr.num_seg, N), dtype=torch.float32, device=dev)
        arg = torch.empty((csr.num_seg, N), dtype=torch.int32, device=dev)
        # a backward will follow: the pool also writes the winners' raw values, which the top
        # GraphNorm's backward statistics then read as a stream instead of gathering h[arg]
        raw = None
        if (POOL_RAW_OUTPUT and any(ctx.needs_input_grad) and N <= 256 and 256 % N == 0
                and _lib.lib.spt_segcsr_max_affine_raw_supported(int(N), R)):
            raw = torch.empty((csr.num_seg, N), dtype=torch.float32, device=dev)
        # same timer key as the plain segment-max: this IS the L0 -> L1 pool launch
        with torch.cuda.device(dev), _timed(f"segcsr_reduce_fwd:3:{R}x{N}"):
            if raw is not None:
                st = _lib.lib.spt_segcsr_max_affine_raw_f32(
                    _lib.ptr(h_last), 1 if store16 else 0, _lib.ptr(csr.perm), _lib.ptr(csr.rowptr),
                    R, csr.num_seg, N, _lib.ptr(am), _lib.ptr(sc), _lib.ptr(bs),
                    float(slope_list[-1]), _lib.ptr(seg_graph), _lib.ptr(out), _lib.ptr(arg),
                    _lib.ptr(raw), _lib.stream_ptr(dev))
            else:
                seg_max = (_lib.lib.spt_segcsr_max_affine_bf16 if store16
                           else _lib.lib.spt_segcsr_max_affine_f32)
                st = seg_max(
                    _lib.ptr(h_last), _lib.ptr(csr.perm), _lib.ptr(csr.rowptr), R, csr.num_seg, N,
                    _lib.ptr(am), _lib.ptr(sc), _lib.ptr(bs), float(slope_list[-1]),
                    _lib.ptr(seg_graph), _lib.ptr(out), _lib.ptr(arg), _lib.stream_ptr(dev))
        _lib.check(st, "spt_segcsr_max_affine")
        ctx.has_raw = raw is not None
        if raw is not None:
            ctx.save_for_backward(arg, *saved, raw)
        else:
            ctx.save_for_backward(arg, *saved)
        ctx.csr = csr
        ctx.seg_graph = seg_graph
        ctx.meta = (len(eps_list), runs, list(slope_list), x.dtype, x.requires_grad,
                    3 if store16 else fmode, store16)
        return out.to(x.dtype)

    @staticmethod
    def _forward_pooled(ctx, x, batch, runs, eps_list, slope_list, csr, seg_graph, params, fmode,
                        store16, mode_top):
        """Layers 0 .. L-2 as a fused chain (their last norm + activation are applied inside the top
        layer's read), then the top layer with the pool in its epilogue
        (``spt_fused_linear_fwd_pool_runs_f32``): out, arg, raw per (segment, channel), the Gram
        totals and the norm's tables - no [rows, N] tensor."""
        L = len(eps_list)
        _, saved_sub, h_prev, (pam, psc, pbs) = _fmlp_forward(
            x, batch, runs, eps_list[:L - 1], slope_list[:L - 1], params[:4 * (L - 1)],
            apply_last=False, fmode=fmode, store16=store16)
        W = _dense(params[4 * (L - 1)].detach(), torch.float32)
        gnw, gnb, gms = (_dense(params[4 * (L - 1) + i].detach(), torch.float32) for i in (1, 2, 3))
        N, K = W.shape
        R = h_prev.shape[0]
        dev = h_prev.device
        B = runs.B
        S = csr.num_seg
        nr, c_r0, c_r1, c_g = runs.c_arrays()
        out = torch.empty((S, N), dtype=torch.float32, device=dev)
        # (the winners' ORIGINAL rows are not asked for: the fused backward and the sparse
        # statistics work on the CSR positions - `arg` would cost one scattered read of perm per
        # (segment, channel): 55 M of them at scene S, 0.17 ms)
        arg = None
        argpos = torch.empty((S, N), dtype=torch.int32, device=dev)
        raw = torch.empty((S, N), dtype=torch.float32, device=dev)
        glen = int(_lib.lib.spt_fused_linear_pool_gram_len(K))
        gram = torch.empty((B, glen), dtype=torch.float64, device=dev)
        mean, rstd, am, sc = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(4))
        nb = _lib.lib.spt_fused_linear_pool_workspace_bytes(K, N)
        ws = _workspace(nb, dev)
        # same timer key as the segment-max it replaces: this IS the L0 -> L1 pool of the step
        with torch.cuda.device(dev), _timed(f"fused_linear_fwd_pool:{K}x{N}:{R}"):
            st = _lib.lib.spt_fused_linear_fwd_pool_runs_f32(
                _lib.ptr(h_prev), _lib.ptr(csr.perm), _lib.ptr(csr.pos_seg()), _lib.ptr(csr.rowptr),
                _lib.ptr(seg_graph), S, R, nr, c_r0, c_r1, c_g, B, K, _lib.ptr(W), N,
                _lib.ptr(gnw), _lib.ptr(gnb), _lib.ptr(gms), float(eps_list[-1]),
                float(slope_list[-1]), _lib.ptr(pam), _lib.ptr(psc), _lib.ptr(pbs),
                float(slope_list[-2]), _lib.ptr(out), _lib.ptr(arg), _lib.ptr(argpos), _lib.ptr(raw),
                _lib.ptr(gram),
                None, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(am), _lib.ptr(sc), mode_top,
                _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "spt_fused_linear_fwd_pool_runs_f32")
        ctx.pool_fused = True
        ctx.n_sub = len(saved_sub)
        ctx.save_for_backward(argpos, raw, gram, mean, rstd, am, sc, W, gnw, gnb, gms, h_prev, pam, psc,
                              pbs, argpos, *saved_sub)
        ctx.csr = csr
        ctx.seg_graph = seg_graph
        ctx.meta = (L, runs, list(slope_list), x.dtype, x.requires_grad,
                    3 if store16 else fmode, store16)
        ctx.mode_top = mode_top
        return out.to(x.dtype)

    @staticmethod
    def _backward_pooled(ctx, gout):
        (arg, raw, gram, mean, rstd, am, sc, W, gnw, gnb, gms, h_prev, pam, psc,
         pbs, argpos) = ctx.saved_tensors[:16]
        saved_sub = ctx.saved_tensors[16:]
        L, runs, slopes, in_dtype, need_gx0, fmode, store16 = ctx.meta
        N, K = W.shape
        R = h_prev.shape[0]
        dev = h_prev.device
        B = runs.B
        csr = ctx.csr
        S = csr.num_seg
        nr, c_r0, c_r1, c_g = runs.c_arrays()
        sp = _lib.stream_ptr(dev)
        gout = _dense(gout, torch.float32)
        with torch.cuda.device(dev):
            # statistics of the top GraphNorm's backward from the pool's sparse gradient
            total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
            rows = _const_tensor(runs.rows_per_graph(), torch.int64, dev)
            nbs = _lib.lib.spt_graphnorm_bwd_stats_sparse_workspace_bytes(S, N, B)
            ws = _workspace(nbs, dev)
            # (`arg` = the CSR positions: the raw variant reads it for the empty-segment sentinel only)
            st = _lib.lib.spt_graphnorm_bwd_stats_sparse_raw_f32(
                _lib.ptr(raw), _lib.ptr(gout), _lib.ptr(arg), _lib.ptr(ctx.seg_graph),
                _lib.ptr(rows), S, R, N, B, _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb),
                float(slopes[-1]), _lib.ptr(total), _lib.ptr(ws), nbs, sp)
            _lib.check(st, "spt_graphnorm_bwd_stats_sparse_raw_f32")
            c1, c2, c3 = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(3))
            gw_n, gb_n, ga_n = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
            st = _lib.lib.spt_graphnorm_bwd_tables_f32(
                _lib.ptr(total), B, N, _lib.ptr(gnw), _lib.ptr(gms), _lib.ptr(mean), _lib.ptr(rstd),
                _lib.ptr(c1), _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(gw_n), _lib.ptr(gb_n),
                _lib.ptr(ga_n), sp)
            _lib.check(st, "spt_graphnorm_bwd_tables_f32")
            gm = torch.empty((S, N), dtype=torch.float32, device=dev)
            gx = torch.empty((R, K), dtype=torch.float32, device=dev)
            gW = torch.empty((N, K), dtype=torch.float32, device=dev)
            # the tables of the norm BELOW (layer L-2's backward) out of this call's post launch
            Ls = L - 1
            sub_tabs, pn, ptot = None, None, None
            if FUSE_POST:
                o = 2 + 5 * Ls
                s_gnw, s_gms = saved_sub[o + Ls + Ls - 1], saved_sub[o + 3 * Ls + Ls - 1]
                s_mean, s_rstd = saved_sub[2 + Ls + 4 * (Ls - 1)], saved_sub[2 + Ls + 4 * (Ls - 1) + 1]
                sub_tabs = (*(torch.empty((B, K), dtype=torch.float32, device=dev) for _ in range(3)),
                            *(torch.empty(K, dtype=torch.float32, device=dev) for _ in range(3)))
                pn = _lib.GnBwdTables(_lib.ptr(s_gnw), _lib.ptr(s_gms), _lib.ptr(s_mean), _lib.ptr(s_rstd),
                                      *[_lib.ptr(t) for t in sub_tabs])
            else:
                ptot = torch.empty((B, 2 * K + 1), dtype=torch.float64, device=dev)
            nb = _lib.lib.spt_fused_linear_pool_workspace_bytes(K, N)
            ws = _workspace(nb, dev)
            args = (_lib.ptr(gout), _lib.ptr(raw), _lib.ptr(argpos), _lib.ptr(csr.perm),
                    _lib.ptr(csr.pos_seg()), _lib.ptr(ctx.seg_graph), S, nr, c_r0, c_r1, c_g, B, N,
                    _lib.ptr(am), _lib.ptr(sc), _lib.ptr(gnb), float(slopes[-1]), _lib.ptr(c1),
                    _lib.ptr(c2), _lib.ptr(c3), _lib.ptr(h_prev), K, _lib.ptr(pam), _lib.ptr(psc),
                    _lib.ptr(pbs), float(slopes[-2]), _lib.ptr(W), _lib.ptr(gram), _lib.ptr(gm),
                    _lib.ptr(gx), _lib.ptr(gW), _lib.ptr(ptot), ctx.mode_top, _lib.ptr(ws), ws.numel())
            with _timed(f"fused_linear_bwd_pool:{K}x{N}:{R}"):
                if pn is not None:
                    st = _lib.lib.spt_fused_linear_bwd_pool_runs_gn_f32(*args, ctypes.addressof(pn), sp)
                else:
                    st = _lib.lib.spt_fused_linear_bwd_pool_runs_f32(*args, sp)
            _lib.check(st, "spt_fused_linear_bwd_pool_runs_f32")
        # layers L-2 .. 0: the fused chain's own backward, entered with the gradient of its
        # normalised output and the statistics (or, FUSE_POST, the tables) of its top norm's backward
        meta_sub = (L - 1, runs, list(slopes[:L - 1]), in_dtype, need_gx0, fmode, store16)
        gx0, grads = _fmlp_backward(saved_sub, meta_sub, gx, top_total=ptot, top_tabs=sub_tabs)
        grads = list(grads) + [gW, gw_n, gb_n, ga_n]
        return (gx0, None, None, None, None, None, None, *grads)

    @staticmethod
    def backward(ctx, gout):
        if ctx.pool_fused:
            return _FusedMLPMaxPool._backward_pooled(ctx, gout)
        arg, saved, raw = ctx.saved_tensors[0], ctx.saved_tensors[1:], None
        if ctx.has_raw:
            saved, raw = saved[:-1], saved[-1]
        L, runs, slopes = ctx.meta[0], ctx.meta[1], ctx.meta[2]
        h_last = saved[2 + L - 1]
        am, sc = saved[2 + L + 4 * (L - 1) + 2], saved[2 + L + 4 * (L - 1) + 3]
        gnb_last = saved[2 + 5 * L + 2 * L + (L - 1)]
        R, N = h_last.shape
        dev = h_last.device
        B = runs.B
        gout = _dense(gout, torch.float32)
        # statistics of the top GraphNorm's backward from the pool's SPARSE gradient (one
        # non-zero per (segment, channel)) instead of a pass over the dense [R, N] tensors
        total = None
        if N <= 256 and 256 % N == 0:
            total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
            rows = _const_tensor(runs.rows_per_graph(), torch.int64, dev)
            nb = _lib.lib.spt_graphnorm_bwd_stats_sparse_workspace_bytes(ctx.csr.num_seg, N, B)
            ws = _workspace(nb, dev)
            with torch.cuda.device(dev):
                if raw is not None:
                    st = _lib.lib.spt_graphnorm_bwd_stats_sparse_raw_f32(
                        _lib.ptr(raw), _lib.ptr(gout), _lib.ptr(arg), _lib.ptr(ctx.seg_graph),
                        _lib.ptr(rows), ctx.csr.num_seg, R, N, B, _lib.ptr(am), _lib.ptr(sc),
                        _lib.ptr(gnb_last), float(slopes[-1]), _lib.ptr(total), _lib.ptr(ws), nb,
                        _lib.stream_ptr(dev))
                else:
                    st = _lib.lib.spt_graphnorm_bwd_stats_sparse_ex_f32(
                        _lib.ptr(h_last), 1 if h_last.dtype == torch.bfloat16 else 0, _lib.ptr(gout),
                        _lib.ptr(arg), _lib.ptr(ctx.seg_graph),
                        _lib.ptr(rows), ctx.csr.num_seg, R, N, B, _lib.ptr(am), _lib.ptr(sc),
                        _lib.ptr(gnb_last), float(slopes[-1]), _lib.ptr(total), _lib.ptr(ws), nb,
                        _lib.stream_ptr(dev))
            _lib.check(st, "spt_graphnorm_bwd_stats_sparse")
        # The pool's gradient has one non-zero per (segment, channel): the top layer's backward
        # reads (gout, arg) through the pool's CSR order instead of a dense [R, N] tensor.  Needs
        # the top GraphNorm's statistics from the sparse route above, an input gradient (L > 1),
        # a built shape, and - with several graphs - graph-contiguous CSR positions (segments
        # numbered graph by graph, as NAG batches are).
        K_top = saved[2 + 5 * L + (L - 1)].shape[1]
        pooled_ok = (total is not None and L > 1
                     and _lib.lib.spt_fused_linear_pooled_supported_ex(int(K_top), int(N), ctx.meta[5]) == 1
                     and runs.sorted_batch
                     and (B == 1 or graph_ranges(ctx.seg_graph, B, ctx.csr.num_seg) is not None))
        if pooled_ok:
            gx0, grads = _fmlp_backward(saved, ctx.meta, None, top_total=total,
                                        pooled=(gout, arg, ctx.csr))
        else:
            gy = _seg_reduce_bwd(gout, arg, ctx.csr, 3, R)
            gx0, grads = _fmlp_backward(saved, ctx.meta, gy, top_total=total)
        return (gx0, None, None, None, None, None, None, *grads)


def fused_mlp(x, batch, num_graphs, layers):
    """``layers``: list of (linear_weight [N,K], gn_weight, gn_bias, gn_mean_scale, eps,
    act_slope) - ``act_slope = 1`` for a layer without activation.  ``batch`` may be sorted
    (clouds of a batch) or piecewise sorted (<= 16 runs of constant id: the edge MLP's norm
    index): every layer is ONE launch per direction over all graphs.  Returns None when
    the fused path does not apply (more runs / graphs than that, unbuilt shape): the caller
    then runs the layer-by-layer HIP path."""
    if x.dim() != 2 or not x.is_cuda:
        return None
    dims = [layers[0][0].shape[1]] + [l[0].shape[0] for l in layers]
    if not fused_mlp_supported(dims):
        return None
    runs = graph_runs(batch, num_graphs if batch is not None else 1, x.shape[0])
    if runs is None:
        return None
    params = [t for l in layers for t in l[:4]]
    return _FusedMLP.apply(x, batch, runs, [l[4] for l in layers], [l[5] for l in layers], *params)


def fused_mlp_maxpool(x, batch, num_graphs, layers, index, num_seg, seg_graph=None):
    """``max-pool(MLP(x), index)`` with the MLP's last GraphNorm + activation applied inside
    the pool's read (``_FusedMLPMaxPool``).  ``seg_graph`` [num_seg]: graph of every segment
    (needed when the batch holds several graphs).  Returns None when the fused path does not
    apply; the caller then runs MLP and pool separately."""
    if x.dim() != 2 or not x.is_cuda:
        return None
    dims = [layers[0][0].shape[1]] + [l[0].shape[0] for l in layers]
    if not fused_mlp_supported(dims) or dims[-1] % 4 != 0:
        return None
    runs = graph_runs(batch, num_graphs if batch is not None else 1, x.shape[0])
    if runs is None or (runs.B > 1 and seg_graph is None):
        return None
    csr = index if isinstance(index, SegmentCSR) else csr_of(index, num_seg)
    sg = None if runs.B <= 1 else _dense(seg_graph, torch.int64, 8)
    params = [t for l in layers for t in l[:4]]
    return _FusedMLPMaxPool.apply(x, batch, runs, [l[4] for l in layers],
                                  [l[5] for l in layers], csr, sg, *params)
