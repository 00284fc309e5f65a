"""Greedy contour-prior partition (``GreedyContourPriorPartition``,
src/transforms/partition.py:383-653; ``merge_components_by_contour_prior_on_data``,
src/utils/components.py:11-130) on the device.

The energy is ``sum_i s_i |x_i - mean(component of i)|^2 + reg * sum_{cut edges} w``.  Starting
from singletons (or from ``data.super_index``), rounds of Boruvka-style merges run until no
component is smaller than ``min_size`` and - unless ``merge_only_small`` - no merge lowers the
energy.  The reference keeps its merge loop in ``torch_graph_components``; the rounds here are
this project's own and ``tests/greedy_partition_reference.py`` restates them in
numpy: the kernels of ``csrc/merge.hip`` and the torch composition below (the route of CPU
tensors) agree with it label for label and bit for bit.

One round, for components with sizes ``S`` int64, feature sums ``F`` f64 and graph ``(E, W)``:

1. ``m = F / S``;
2. per edge ``g = f32(S_a S_b / (S_a + S_b) * |m_a - m_b|^2 - reg * w)``, in f64;
3. every component takes the neighbour with the least ``(g, id)``;
4. it is active iff it has an edge and (``S < min_size``, or ``g < 0`` unless ``merge_only_small``);
5. ``parent`` = the choice of an active component, itself otherwise, the smaller of a mutual
   pair its own parent; pointer jumping to the roots;
6. roots relabelled in ascending order;
7. sizes and sums accumulated over the members in ascending id;
8. the graph's quotient under the relabelling (``component_graph``).

Host reads per round, three: the active count (ends the level), the new component count
together with the flag of the last jump pass, the new edge count.
"""
import math

import torch

from . import _lib
from .ops import _workspace

__all__ = ["component_graph", "edge_lengths", "edge_weights", "merge_components_by_contour_prior",
           "merge_components_by_contour_prior_on_data", "check_edge_weight_mode", "EDGE_WEIGHT_MODES",
           "REDUCES"]

REDUCES = {"add": 0, "mean": 1, "max": 2, "min": 3, "mul": 4}
EDGE_WEIGHT_MODES = ("unit", "inverse_distance", "exp_neg_distance", "exp_neg_latent_distance",
                     "affinity_latent_distance", "affinity_latent_distance_exp_neg")
LONG_RUN = 512              # longer sums: 64 strided partial sums + the xor tree (csrc/merge.hip)
MAX_SIZE = 1 << 29          # f64(x) * s stays exact: 24 + 29 bits
MAX_NODES = (1 << 31) - 4096
_NO_CHOICE = torch.iinfo(torch.int64).max


def _check_reduce(reduce):
    if reduce not in REDUCES:
        raise ValueError(f"reduce must be one of {sorted(REDUCES)}, got {reduce!r}")


# ---------------------------------------------------------------------------
# torch composition: the route of CPU tensors, and the yardstick of the bench
# ---------------------------------------------------------------------------
def _combine(reduce, a, b):
    if reduce == "max":
        return torch.where(b > a, b, a)
    if reduce == "min":
        return torch.where(b < a, b, a)
    if reduce == "mul":
        return a * b
    return a + b


def _ordered_reduce(vals, ptr, reduce, from_zero):
    """Per group ``g`` = rows ``ptr[g] .. ptr[g + 1]`` of ``vals`` (already in group order): the
    reduction in exactly the kernels' order.  Up to ``LONG_RUN`` rows serially (from 0 when
    ``from_zero``, else from the first row); longer groups as 64 strided partial results combined
    by the xor tree 32, 16, .., 1.  'mean' divides the sum by the row count in ``vals``' type."""
    G = ptr.numel() - 1
    start, lens = ptr[:-1], ptr[1:] - ptr[:-1]
    tail = vals.shape[1:]
    out = torch.zeros((G,) + tuple(tail), dtype=vals.dtype, device=vals.device)
    if G == 0:
        return out
    expand = (lambda m: m.view(-1, *([1] * len(tail))))
    short = lens <= LONG_RUN
    first = 0 if from_zero else 1
    if not from_zero:
        has = lens > 0
        out[has] = vals[start[has]]
    top = int(lens[short].max()) if bool(short.any()) else 0
    for k in range(first, top):
        sel = (short & (lens > k)).nonzero().view(-1)
        out[sel] = _combine(reduce, out[sel], vals[start[sel] + k])
    lanes = torch.arange(64, device=vals.device)
    for g in (~short).nonzero().view(-1).tolist():
        seg = vals[int(start[g]):int(start[g]) + int(lens[g])]
        part = torch.zeros((64,) + tuple(tail), dtype=vals.dtype, device=vals.device) if from_zero \
            else seg[:64].clone()
        for k in range(first, -(-seg.shape[0] // 64)):
            chunk = seg[64 * k:64 * k + 64]
            part[:chunk.shape[0]] = _combine(reduce, part[:chunk.shape[0]], chunk)
        for o in (32, 16, 8, 4, 2, 1):
            part = _combine(reduce, part, part[lanes ^ o])
        out[g] = part[0]
    if reduce == "mean":
        out = out / expand(lens.to(vals.dtype))
    return out


def _orderable_bits(g):
    """int64 in [0, 2^32): the f32 bits of ``g`` in an order that is the floats' (-0.0 as +0.0)."""
    u = (g + 0.0).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return torch.where((u & 0x80000000) != 0, (~u) & 0xFFFFFFFF, u | 0x80000000)


class _Torch:
    """Every step of a round from torch calls, in the kernels' arithmetic and order."""

    @staticmethod
    def component_graph(index, edge_index, edge_attr, reduce, num_nodes, num_components):
        dev = edge_index.device
        a, b = edge_index[0].long(), edge_index[1].long()
        if a.numel() and (int(torch.minimum(a.min(), b.min())) < 0
                          or int(torch.maximum(a.max(), b.max())) >= num_nodes):
            raise ValueError("edge_index holds node ids out of range")
        w = torch.ones(a.numel(), dtype=torch.float32, device=dev) if edge_attr is None \
            else edge_attr.float()
        if index is not None:
            a, b = index[a], index[b]
        lo, hi = torch.minimum(a, b), torch.maximum(a, b)
        keep = (lo != hi).nonzero().view(-1)                     # ascending: the input order stays
        key = (lo[keep] << 32) | hi[keep]
        key, order = torch.sort(key, stable=True)
        w = w[keep][order]
        head = torch.ones(key.numel(), dtype=torch.bool, device=dev)
        head[1:] = key[1:] != key[:-1]
        first = head.nonzero().view(-1)
        ptr = torch.cat([first, torch.tensor([key.numel()], device=dev)])
        ukey = key[first]
        out_w = _ordered_reduce(w, ptr, reduce, from_zero=False)
        return torch.stack([ukey >> 32, ukey & 0xFFFFFFFF]), out_w

    @staticmethod
    def gains(F, S, E, W, reg):
        m = F / S.double()[:, None]
        a, b = E[0], E[1]
        ma, mb = m[a], m[b]
        d2 = torch.zeros(a.numel(), dtype=torch.float64, device=F.device)
        for d in range(F.shape[1]):
            t = ma[:, d] - mb[:, d]
            d2 = d2 + t * t
        sa, sb = S[a].double(), S[b].double()
        return (((sa * sb) / (sa + sb)) * d2 - float(reg) * W.double()).float()

    @classmethod
    def choose(cls, F, S, E, W, reg):
        C = S.numel()
        a, b = E[0], E[1]
        ob = _orderable_bits(cls.gains(F, S, E, W, reg)) << 31        # ids < 2^31: 63 bits in all
        best = torch.full((C,), _NO_CHOICE, dtype=torch.int64, device=S.device)
        best.scatter_reduce_(0, torch.cat([a, b]), torch.cat([ob | b, ob | a]), "amin")
        return best

    @staticmethod
    def resolve(best, S, min_size, merge_only_small):
        ar = torch.arange(S.numel(), device=S.device)
        has = best != _NO_CHOICE
        partner = torch.where(has, best & 0x7FFFFFFF, ar)
        active = has & (S < min_size)
        if not merge_only_small:
            active |= has & ((best >> 31) < 0x80000000)              # g < 0
        mutual = active & active[partner] & (partner[partner] == ar)
        parent = torch.where(active & ~(mutual & (ar < partner)), partner, ar)
        return parent, int(active.sum())

    @staticmethod
    def relabel(parent):
        while True:
            nxt = parent[parent]
            if bool((nxt == parent).all()):
                break
            parent = nxt
        roots, label = torch.unique(parent, return_inverse=True)
        return label, roots.numel()

    @staticmethod
    def accumulate(label, num_new, S, F, Q):
        order = torch.sort(label, stable=True).indices
        ptr = torch.zeros(num_new + 1, dtype=torch.int64, device=label.device)
        ptr[1:] = torch.cumsum(torch.bincount(label, minlength=num_new), 0)
        S2 = torch.zeros(num_new, dtype=torch.int64, device=label.device).index_add_(0, label, S)
        F2 = _ordered_reduce(F[order], ptr, "add", from_zero=True)
        Q2 = None if Q is None else _ordered_reduce(Q[order], ptr, "add", from_zero=True)
        return S2, F2, Q2

    @staticmethod
    def edge_lengths(rows, edge_index):
        n = rows.shape[0]
        a, b = edge_index[0], edge_index[1]
        if a.numel() and (int(torch.minimum(a.min(), b.min())) < 0
                          or int(torch.maximum(a.max(), b.max())) >= n):
            raise ValueError("edge_index holds node ids out of range")
        ra, rb = rows[a].double(), rows[b].double()
        d2 = torch.zeros(a.numel(), dtype=torch.float64, device=rows.device)
        for c in range(rows.shape[1]):
            t = ra[:, c] - rb[:, c]
            d2 = d2 + t * t
        dist = d2.sqrt().float()
        return dist, float(dist.double().sum())


# ---------------------------------------------------------------------------
# csrc/merge.hip
# ---------------------------------------------------------------------------
class _Kernels:
    @staticmethod
    def component_graph(index, edge_index, edge_attr, reduce, num_nodes, num_components):
        L = _lib.lib
        dev = edge_index.device
        ei = _lib.dense(edge_index, torch.int64, 8)
        E = ei.shape[1]
        w = _lib.dense(edge_attr, torch.float32, 4)
        index = _lib.dense(index, torch.int64, 8)
        out_e = torch.empty((2, E), dtype=torch.int64, device=dev)
        out_w = torch.empty(E, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        nbytes = L.spt_component_graph_workspace_bytes(E)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = L.spt_component_graph_f32(
                _lib.ptr(ei), E, E, _lib.ptr(w), _lib.ptr(index), num_nodes, num_components,
                REDUCES[reduce], _lib.ptr(out_e), E, _lib.ptr(out_w), _lib.ptr(counts),
                _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_component_graph_f32")
        n_out, bad = counts.tolist()                                  # host read: output size
        if bad:
            raise ValueError("edge_index holds node ids out of range")
        return out_e[:, :n_out].contiguous(), out_w[:n_out]

    @staticmethod
    def choose(F, S, E, W, reg, gain=None):
        L = _lib.lib
        dev = F.device
        C, D = F.shape
        m = torch.empty_like(F)
        best = torch.empty(max(C, 1), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = L.spt_merge_means_f64(_lib.ptr(F), _lib.ptr(S), C, D, _lib.ptr(m),
                                       _lib.stream_ptr(dev))
            _lib.check(st, "spt_merge_means_f64")
            st = L.spt_merge_choose_f64(_lib.ptr(m), _lib.ptr(S), C, D, _lib.ptr(E), E.shape[1],
                                        E.shape[1], _lib.ptr(W), float(reg), _lib.ptr(best),
                                        _lib.ptr(gain), _lib.stream_ptr(dev))
        _lib.check(st, "spt_merge_choose_f64")
        return best

    @staticmethod
    def resolve(best, S, min_size, merge_only_small):
        dev = S.device
        C = S.numel()
        parent = torch.empty(max(C, 1), dtype=torch.int64, device=dev)
        active = torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            st = _lib.lib.spt_merge_resolve(_lib.ptr(best), _lib.ptr(S), C, int(min_size),
                                            int(bool(merge_only_small)), _lib.ptr(parent),
                                            _lib.ptr(active), _lib.stream_ptr(dev))
        _lib.check(st, "spt_merge_resolve")
        return parent[:C], int(active)                                # host read: ends the level

    @staticmethod
    def relabel(parent):
        L = _lib.lib
        dev = parent.device
        C = parent.numel()
        other = torch.empty_like(parent)
        state = torch.empty(2, dtype=torch.int64, device=dev)        # jump flag, new count
        label = torch.empty(C, dtype=torch.int64, device=dev)
        roots = torch.empty(max(C, 1), dtype=torch.int64, device=dev)
        nbytes = L.spt_relabel_consecutive_workspace_bytes(C)
        ws = _workspace(nbytes, dev)
        # a forest of C nodes is at most C - 1 deep and a pass halves the depth: after
        # ceil(log2 C) passes every entry is a root, and one more pass reports that nothing moved
        passes = max(1, math.ceil(math.log2(max(C, 2)))) + 1
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            for p in range(passes):
                last = p == passes - 1
                st = L.spt_merge_jump(_lib.ptr(parent), C, _lib.ptr(other),
                                      _lib.ptr(state) if last else None, stream)
                _lib.check(st, "spt_merge_jump")
                parent, other = other, parent
            st = L.spt_relabel_consecutive(_lib.ptr(parent), None, C, C, _lib.ptr(label),
                                           _lib.ptr(roots), state.data_ptr() + 8, _lib.ptr(ws),
                                           nbytes, stream)
        _lib.check(st, "spt_relabel_consecutive")
        changed, num_new = state.tolist()                             # host read: new size
        if changed:
            raise RuntimeError("pointer jumping did not reach the roots: the parents held a cycle")
        return label, num_new

    @staticmethod
    def accumulate(label, num_new, S, F, Q):
        L = _lib.lib
        dev = F.device
        C, D = F.shape
        S2 = torch.empty(num_new, dtype=torch.int64, device=dev)
        F2 = torch.empty((num_new, D), dtype=torch.float64, device=dev)
        Q2 = None if Q is None else torch.empty((num_new, 3), dtype=torch.float64, device=dev)
        nbytes = L.spt_merge_accumulate_workspace_bytes(C, num_new)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = L.spt_merge_accumulate_f64(_lib.ptr(label), C, num_new, _lib.ptr(S), _lib.ptr(F), D,
                                            _lib.ptr(Q), _lib.ptr(S2), _lib.ptr(F2), _lib.ptr(Q2),
                                            _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_merge_accumulate_f64")
        return S2, F2, Q2

    @staticmethod
    def edge_lengths(rows, edge_index):
        L = _lib.lib
        dev = rows.device
        rows = _lib.dense(rows, torch.float32, 4)
        ei = _lib.dense(edge_index, torch.int64, 8)
        n, cols = rows.shape
        E = ei.shape[1]
        dist = torch.empty(E, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)         # the sum; the bad count's bits
        nbytes = L.spt_edge_weights_workspace_bytes(E)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            st = L.spt_edge_weights_f32(_lib.ptr(rows), n, cols, cols, _lib.ptr(ei), E, E,
                                        _lib.ptr(dist), _lib.ptr(out), out.data_ptr() + 8,
                                        _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
        _lib.check(st, "spt_edge_weights_f32")
        host = out.cpu()                                              # host read
        total = float(host[0])
        if int(host[1:].view(torch.int64)):
            raise ValueError("edge_index holds node ids out of range")
        return dist, total


def _route(t, route):
    if route is None:
        route = "kernels" if t.is_cuda else "torch"
    if route == "kernels":
        _lib.require_cuda(t)
        return _Kernels
    if route == "torch":
        return _Torch
    raise ValueError(f"route must be 'kernels' or 'torch', got {route!r}")


# ---------------------------------------------------------------------------
# public functions
# ---------------------------------------------------------------------------
def component_graph(index, edge_index, edge_attr=None, reduce="add", num_components=None,
                    route=None):
    """Graph of the components ``index`` [N] of the nodes of ``edge_index`` [2, E] (any order,
    both directions, duplicates, self loops): both ends relabelled, every pair ordered lo < hi,
    lo == hi dropped, sorted by (lo, hi), equal pairs merged with ``reduce`` ('add', 'mean',
    'max', 'min', 'mul') in f32, serially in the order of the input positions (more than 512
    duplicates: 64 strided partial results and the xor tree).  ``index=None`` is the identity
    over ``num_components`` nodes; ``edge_attr=None`` counts as ones.  Returns ``(edge_index
    [2, E'] int64, edge_attr [E'] f32)``."""
    _check_reduce(reduce)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    if index is None:
        if num_components is None:
            raise ValueError("index=None needs num_components (the number of nodes)")
        num_nodes = num_components = int(num_components)
    else:
        num_nodes = index.numel()
        if num_components is None:
            num_components = int(index.max()) + 1 if num_nodes else 0
        index = index.long()
    if max(num_nodes, num_components, edge_index.shape[1]) >= MAX_NODES:
        raise ValueError("the partition takes fewer than 2^31 nodes and edges")
    if edge_attr is not None and edge_attr.shape != (edge_index.shape[1],):
        raise ValueError("edge_attr must be [E]")
    return _route(edge_index, route).component_graph(index, edge_index.long(), edge_attr, reduce,
                                                     num_nodes, int(num_components))


def edge_lengths(rows, edge_index, route=None):
    """``(dist, total)``: ``dist[e] = f32(sqrt(sum_c (rows[a, c] - rows[b, c])^2))`` with the
    squares summed from column 0 in f64, and the f64 sum of ``dist`` (a python float)."""
    if rows.dim() != 2 or rows.shape[1] < 1:
        raise ValueError("rows must be [N, C] with C >= 1")
    return _route(rows, route).edge_lengths(rows.float(), edge_index.long())


def check_edge_weight_mode(mode):
    """Raises for a mode that is unknown or refused (the two 'affinity' modes)."""
    if mode not in EDGE_WEIGHT_MODES:
        raise ValueError(f"Invalid edge weight mode: {mode}.\nValid options are: "
                         f"{list(EDGE_WEIGHT_MODES)}")
    if mode == "affinity_latent_distance":
        raise NotImplementedError(
            "'affinity_latent_distance' reads `epsilon_edge_weight`, which the reference never "
            "sets (partition.py:630-634): the mode cannot run there either")
    if mode == "affinity_latent_distance_exp_neg":
        raise ValueError(f"Invalid edge weight mode: {mode} (the reference lists it and raises, "
                         "partition.py:635-638)")


def edge_weights(pos, x, edge_index, mode="unit", d_0=None, route=None):
    """Edge weights of ``GreedyContourPriorPartition.edge_weights`` (partition.py:585-640), f32:
    'unit' 1; 'inverse_distance' ``1 / (1 + d / d_0)``; 'exp_neg_distance' ``exp(-d / d_0)``, both
    with the edge length in ``pos``; 'exp_neg_latent_distance' the same with the length in ``x``.
    ``d_0=None``: the mean length, f32 of an f64 sum over the edges.  (The reference's 'unit' mode
    makes int64 ones.)"""
    check_edge_weight_mode(mode)
    E = edge_index.shape[1]
    if mode == "unit":
        return torch.ones(E, dtype=torch.float32, device=edge_index.device)
    name, rows = ("x", x) if mode == "exp_neg_latent_distance" else ("pos", pos)
    if rows is None:
        raise ValueError(f"mode {mode!r} needs {name}")
    if rows.dim() == 1:
        rows = rows.view(-1, 1)
    dist, total = edge_lengths(rows, edge_index, route)
    if d_0 is None:
        d_0 = total / E if E else 1.0
    d_0 = torch.tensor(float(d_0), dtype=torch.float32, device=dist.device)
    if mode == "inverse_distance":
        return 1 / (1 + dist / d_0)
    return torch.exp(-dist / d_0)


def merge_components_by_contour_prior(X, S, E, W, reg, min_size, merge_only_small=False,
                                      max_iterations=-1, reduce="add", P=None, k=0, route=None):
    """Greedy merge of the components ``X`` [C, D] f32 (mean features), ``S`` [C] int64 (sizes)
    linked by ``E`` [2, E] with weights ``W`` [E] (None = ones), until no component below
    ``min_size`` has an edge and - unless ``merge_only_small`` - no edge has a negative gain, or
    for ``max_iterations`` rounds when that is positive.  ``P`` [C, 3]: mean positions, carried
    along for the output.

    Returns ``(I_merged [C] int64, iterations, (X_merged f32, S_merged int64, E_cp [2, E'],
    W_cp f32, P_merged f32 or None))`` as ``torch_graph_components`` does for the reference
    (components.py:98-113).  ``route``: 'kernels' (CUDA tensors, the default there) or 'torch'."""
    _check_reduce(reduce)
    if k > 0:
        raise NotImplementedError("k > 0 (reconnecting isolated components every round) is not built")
    if X.dim() == 1:
        X = X.view(-1, 1)
    C, D = X.shape
    if D < 1:
        raise ValueError("X needs at least one column")
    if C >= MAX_NODES:
        raise ValueError("the partition takes fewer than 2^31 components")
    S = S.long().contiguous()
    if S.shape != (C,):
        raise ValueError("S must be [C]")
    if C and (int(S.max()) >= MAX_SIZE or int(S.min()) < 1):
        raise ValueError("sizes must lie in [1, 2^29)")
    B = _route(X, route)
    F = (X.double() * S.double()[:, None]).contiguous()
    Q = None if P is None else (P.double() * S.double()[:, None]).contiguous()
    E, W = component_graph(None, E, W, reduce, num_components=C, route=route)
    I = torch.arange(C, device=X.device)
    iterations = 0
    while E.shape[1] and not (0 < max_iterations <= iterations):
        best = B.choose(F, S, E, W, reg)
        parent, n_active = B.resolve(best, S, min_size, merge_only_small)
        if n_active == 0:
            break
        label, num_new = B.relabel(parent)
        S, F, Q = B.accumulate(label, num_new, S, F, Q)
        E, W = B.component_graph(label, E, W, reduce, label.numel(), num_new)
        I = label[I]
        iterations += 1
    Sd = S.double()[:, None]
    X_merged = (F / Sd).float()
    P_merged = None if Q is None else (Q / Sd).float()
    return I, iterations, (X_merged, S, E, W, P_merged)


def merge_components_by_contour_prior_on_data(data, reg, min_size, merge_only_small=False, k=-1,
                                              w_adjacency=-1, max_iterations=-1, sharding=None,
                                              reduce="add", verbose=False, route=None):
    """``merge_components_by_contour_prior_on_data`` of the reference (components.py:11-130):
    merges the nodes of ``data`` (``x``, ``pos``, ``edge_index``, ``edge_attr``, optional
    ``node_size``), or the components ``data.super_index`` when it has one, and returns
    ``(data, (X_merged, S_merged, E_cp, W_cp, P_merged, sub))``: a clone of ``data`` whose
    ``super_index`` names the merged component of every node, and ``sub``, the ``Cluster`` of the
    merged components with ascending node ids inside each.  ``sharding`` and ``verbose`` are
    accepted and ignored; ``k > 0`` is refused."""
    from .data import Cluster
    if k > 0:
        raise NotImplementedError("k > 0 (reconnecting isolated components every round) is not built")
    for key in ("x", "pos", "edge_index", "edge_attr"):
        if data.get(key) is None:
            raise ValueError(f"data.{key} is required")
    X, P, E, W = data.x, data.pos, data.edge_index, data.edge_attr
    if X.dim() == 1:
        X = X.view(-1, 1)
    N = X.shape[0]
    dev = X.device
    B = _route(X, route)
    S = data.get("node_size")
    S = torch.ones(N, dtype=torch.int64, device=dev) if S is None else S.long().view(-1)
    I0 = data.get("super_index")
    if I0 is None:
        X_cp, P_cp, S_cp = X.float(), P.float(), S
        I0 = None
    else:
        # the components' sizes and size-weighted means by the rules of a round: sums over the
        # members in ascending id, in f64
        I0 = I0.long().contiguous()
        C0 = int(I0.max()) + 1 if N else 0
        if N and (int(S.max()) >= MAX_SIZE or int(S.min()) < 1):
            raise ValueError("sizes must lie in [1, 2^29)")
        if N and int(torch.bincount(I0, minlength=C0).min()) == 0:
            raise ValueError("data.super_index must use every id up to its maximum")
        Sd = S.double()[:, None]
        S_cp, F_cp, Q_cp = B.accumulate(I0, C0, S.contiguous(), (X.double() * Sd).contiguous(),
                                        (P.double() * Sd).contiguous())
        X_cp = (F_cp / S_cp.double()[:, None]).float()
        P_cp = (Q_cp / S_cp.double()[:, None]).float()
        E, W = component_graph(I0, E, W, reduce, num_components=C0, route=route)
    I_merged, _, (X_m, S_m, E_cp, W_cp, P_m) = merge_components_by_contour_prior(
        X_cp, S_cp, E, W, reg, min_size, merge_only_small=merge_only_small,
        max_iterations=max_iterations, reduce=reduce, P=P_cp, route=route)
    data = data.clone()
    super_index = I_merged if I0 is None else I_merged[I0]
    data.super_index = super_index
    C = S_m.numel()
    if super_index.is_cuda:
        from .csr import build_csr
        csr = build_csr(super_index, max(C, 1))
        pointers, points = csr.rowptr.long()[:C + 1], csr.perm.long()
    else:
        points = torch.sort(super_index, stable=True).indices
        pointers = torch.zeros(C + 1, dtype=torch.int64)
        pointers[1:] = torch.cumsum(torch.bincount(super_index, minlength=C), 0)
    sub = Cluster(pointers, points, ascending=True)
    return data, (X_m, S_m, E_cp, W_cp, P_m, sub)
