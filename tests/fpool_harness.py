"""Shared by tests/test_fpool_fwd_level_gpu.py and tests/test_pool_scene_size_gpu.py: builds a
pool-fused forward problem with the edges the kernel has to get right, calls the C entry
spt_fused_linear_fwd_pool_runs_f32 with NaN / -1 pre-filled outputs, and checks every output
against tests/fpool_reference.py (f64, on the GPU, in row chunks).

The problem (`build`):
  * empty segments at the front (0, 1), at the back (last two), 1 % at random in between, and - the
    first and the last segment of every run - on both sides of the graph boundaries;
  * optionally one GIANT segment (the wave that cuts into it walks all of it; the waves whose
    nominal ranges it swallows are left without rows);
  * one segment with a block of 24 bitwise equal rows (more than a tile) whose h is extreme in
    about half of the channels: the first of them has to win;
  * 40 channels with negative norm weight (the pool is a min there), 3 with weight exactly 0;
  * three graphs: the middle run is ~100 segments (a few thousand rows: less than one workgroup's
    share of a large run), the run boundaries are not multiples of 16 rows.
"""
import ctypes
from dataclasses import dataclass

import torch

import fpool_reference as R
from superpoint_transformer_amd import _lib, synthetic

X_BF16 = 16                      # SPT_FMLP_X_BF16 (include/spt_hip.h)
QUANTITIES = ("raw", "out", "G", "sum_y", "sum_h", "sum_h2", "mean", "rstd", "am", "scale")
DUP_ROWS, DUP_SIZE, DUP_AT = 24, 60, 5


@dataclass
class Case:
    pb: R.Problem
    num_seg: int
    perm32: torch.Tensor          # None: rows in CSR order
    pos_seg: torch.Tensor
    rowptr32: torch.Tensor
    dup_seg: int
    giant_seg: int                # -1: none
    K: int
    N: int


def build(gen, rows, num_seg, K, N, dev, order, graphs, giant=0, in16=False, short_run=100):
    empty = torch.zeros(num_seg, dtype=torch.bool, device=dev)
    empty[[0, 1, num_seg - 2, num_seg - 1]] = True
    empty |= torch.rand(num_seg, generator=gen, device=dev) < 0.01
    if graphs == 3:
        sA = num_seg * 11 // 20
        sB = sA + short_run
        bounds = [0, sA, sB, num_seg]
    elif graphs == 2:
        bounds = [0, num_seg * 9 // 20, num_seg]
    else:
        bounds = [0, num_seg]
    for s in bounds[1:-1]:                                   # last segment of a run, first of the next
        empty[s - 1] = True
        empty[s] = True
    dup_seg, giant_seg = num_seg // 2 + 7 if graphs != 3 else bounds[1] + short_run // 2, -1
    empty[dup_seg] = False
    special = DUP_SIZE
    if giant:
        giant_seg = num_seg // 4
        empty[giant_seg] = False
        special += giant
    normal = ~empty
    normal[dup_seg] = False
    if giant:
        normal[giant_seg] = False
    sizes = torch.zeros(num_seg, dtype=torch.long, device=dev)
    sizes[normal] = synthetic._segment_sizes(gen, rows - special, int(normal.sum()), "lognormal", dev)
    sizes[dup_seg] = DUP_SIZE
    if giant:
        sizes[giant_seg] = giant
    # run boundaries off the 16-row grid: move single rows across a boundary until they are
    while any(int(sizes[:s].sum()) % 16 == 0 for s in bounds[1:-1]):
        big = torch.nonzero(sizes[:bounds[1]] > 2).flatten()
        sizes[big[0]] -= 1
        sizes[num_seg - 3] += 1
    rowptr = torch.zeros(num_seg + 1, dtype=torch.long, device=dev)
    rowptr[1:] = torch.cumsum(sizes, 0)
    assert int(rowptr[-1]) == rows
    runs = [(int(rowptr[a]), int(rowptr[b]), i) for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
    assert all(p0 % 16 for p0, _, _ in runs[1:])
    seg_graph = None
    if graphs > 1:
        seg_graph = torch.zeros(num_seg, dtype=torch.long, device=dev)
        for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
            seg_graph[a:b] = i
    si = torch.repeat_interleave(torch.arange(num_seg, device=dev), sizes)
    if order == "shuffled":
        si = si[torch.randperm(rows, generator=gen, device=dev)]
        perm = torch.argsort(si, stable=True)
        pos_seg = si[perm].int()
    else:
        perm, pos_seg = None, si.int()
    del si
    x = torch.randn(rows, K, device=dev, generator=gen) * 1.5 + 0.3
    dpos = torch.arange(DUP_AT, DUP_AT + DUP_ROWS, device=dev) + rowptr[dup_seg]
    drows = dpos if perm is None else perm[dpos]
    x[drows] = 4 * x[drows[0]]
    if in16:
        x = x.bfloat16()
    W = torch.randn(N, K, device=dev, generator=gen) * 0.1
    gnw = torch.randn(N, device=dev, generator=gen).abs() + 0.05
    pick = torch.randperm(N, generator=gen, device=dev)
    gnw[pick[:40]] = -gnw[pick[:40]]
    gnw[pick[40:43]] = 0.0
    gnb = torch.randn(N, device=dev, generator=gen) * 0.1
    gms = torch.rand(N, device=dev, generator=gen)
    pam = torch.randn(graphs, K, device=dev, generator=gen) * 0.1
    psc = torch.rand(graphs, K, device=dev, generator=gen) + 0.5
    pbs = torch.randn(K, device=dev, generator=gen) * 0.1
    pb = R.Problem(x=x, perm=perm, rowptr=rowptr, runs=runs, seg_graph=seg_graph, W=W, pre_am=pam,
                   pre_scale=psc, pre_bias=pbs, pre_slope=0.2, gn_weight=gnw, gn_bias=gnb,
                   gn_mean_scale=gms, eps=1e-5, slope=0.01)
    return Case(pb, num_seg, None if perm is None else perm.int(), pos_seg, rowptr.int(), dup_seg,
                giant_seg, K, N)


@dataclass
class Outputs:
    status: int
    out: torch.Tensor
    arg: torch.Tensor
    argpos: torch.Tensor
    raw: torch.Tensor
    gram: torch.Tensor
    total: torch.Tensor
    mean: torch.Tensor
    rstd: torch.Tensor
    am: torch.Tensor
    scale: torch.Tensor


def call_forward(case, mode, want_arg=True):
    """One call of the C entry; every output pre-filled with NaN / -1."""
    pb, S, K, N = case.pb, case.num_seg, case.K, case.N
    dev, B = pb.x.device, pb.num_graphs
    assert (pb.x.dtype == torch.bfloat16) == bool(mode & X_BF16) and pb.x.shape == (pb.n_rows, K)
    assert pb.x.is_contiguous() and case.pos_seg.numel() == pb.n_rows and case.rowptr32.numel() == S + 1
    nan = float("nan")
    out, raw = (torch.full((S, N), nan, device=dev) for _ in range(2))
    arg, argpos = (torch.full((S, N), -1, dtype=torch.int32, device=dev) for _ in range(2))
    glen = int(_lib.lib.spt_fused_linear_pool_gram_len(K))
    gram = torch.full((B, glen), nan, dtype=torch.float64, device=dev)
    total = torch.full((B, 2 * N + 1), nan, dtype=torch.float64, device=dev)
    mean, rstd, am, sc = (torch.full((B, N), nan, device=dev) for _ in range(4))
    ws = torch.empty(_lib.lib.spt_fused_linear_pool_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    n = len(pb.runs)
    r0 = (ctypes.c_int64 * n)(*[r[0] for r in pb.runs])
    r1 = (ctypes.c_int64 * n)(*[r[1] for r in pb.runs])
    rg = (ctypes.c_int32 * n)(*[r[2] for r in pb.runs])
    P = _lib.ptr
    opt = lambda t: None if t is None else P(t)
    st = _lib.lib.spt_fused_linear_fwd_pool_runs_f32(
        P(pb.x), opt(case.perm32), P(case.pos_seg), P(case.rowptr32), opt(pb.seg_graph), S, pb.n_rows, n,
        r0, r1, rg, B, K, P(pb.W), N, P(pb.gn_weight), P(pb.gn_bias), P(pb.gn_mean_scale), pb.eps, pb.slope,
        P(pb.pre_am), P(pb.pre_scale), P(pb.pre_bias), pb.pre_slope, P(out), P(arg) if want_arg else None,
        P(argpos), P(raw), P(gram), P(total), P(mean), P(rstd), P(am), P(sc), mode, P(ws), ws.numel(),
        _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return Outputs(st, out, arg, argpos, raw, gram, total, mean, rstd, am, sc)


def _rel(a, r):
    return float((a.to(R.D) - r).abs().max() / r.abs().max())


def _nanmax(*v):
    """max that keeps a NaN (Python's max drops it)."""
    return float("nan") if any(e != e for e in v) else max(v)


def check_forward(case, mode, o, label, parent=None, factor=2.0, subset=None):
    """All properties of one forward call's outputs `o`.  Prints the measured figures first, then
    asserts: the exact properties always, the error bounds against `factor` x `parent` (a dict
    quantity -> the parent commit's measured error); parent None only measures.  `subset`: segment
    ids on which the per-segment reference is evaluated once more on its own (the way a caller
    with no room for all segments would) and compared in full.  Returns the measured errors."""
    pb, S, N, K = case.pb, case.num_seg, case.N, case.K
    dev, n_rows, B = pb.x.device, pb.n_rows, pb.num_graphs
    pb.bf16 = (mode & 3) == 3
    _lib.check(o.status, "spt_fused_linear_fwd_pool_runs_f32")
    st = R.statistics(pb)
    ref = R.pool_segments(pb, st, torch.arange(S, device=dev), witness=o.argpos)
    rp = pb.rowptr
    a0, a1 = rp[:-1, None], rp[1:, None]
    live = (a1 > a0).expand(S, N)
    sgn = torch.where(pb.gn_weight < 0, -1.0, 1.0).to(R.D)
    zero_w = pb.gn_weight == 0
    ap = o.argpos.long()
    in_range = (ap >= a0) & (ap < a1)

    errs = {}
    errs["raw"] = float((o.raw.to(R.D) - ref.h_witness)[live].abs().max()) / st.h_absmax
    errs["out"] = _rel(o.out, ref.out)
    deficit = float((ref.ext - sgn * ref.h_witness)[live].max()) / st.h_absmax
    per_graph = {q: [] for q in QUANTITIES[2:]}
    for b in range(B):
        per_graph["G"].append(_rel(o.gram[b, :K * K], st.gram[b, :K * K]))
        per_graph["sum_y"].append(_rel(o.gram[b, K * K:K * K + K], st.gram[b, K * K:K * K + K]))
        per_graph["sum_h"].append(_rel(o.total[b, :N], st.total[b, :N]))
        per_graph["sum_h2"].append(_rel(o.total[b, N:2 * N], st.total[b, N:2 * N]))
        for q in ("mean", "rstd", "am", "scale"):
            per_graph[q].append(_rel(getattr(o, q)[b], getattr(st, q)[b]))
    for q, v in per_graph.items():
        errs[q] = max(v) if all(e == e for e in v) else float("nan")
    print(f"fpool fwd {label}: " + " ".join(f"{q} {errs[q]:.3e}" for q in QUANTITIES) +
          f" | witness-deficit {deficit:.3e} max|h| {st.h_absmax:.4f}")

    # ---- exact properties ------------------------------------------------------------------------
    assert all(e == e for e in errs.values()), f"NaN / unwritten element in an output: {errs}"
    assert bool(in_range[live].all()), "an arg position outside its segment"
    dead = ~live
    assert bool((ap[dead] == n_rows).all()) and bool((o.raw[dead] == 0).all()) and bool((o.out[dead] == 0).all())
    for b in range(B):
        nb = sum(p1 - p0 for p0, p1, g in pb.runs if g == b)
        assert o.gram[b, K * K + K].item() == nb and o.total[b, 2 * N].item() == nb
    # zero-weight channels: exactly the segment's first position
    lz = live[:, 0]
    assert bool((ap[lz][:, zero_w] == a0[lz]).all()), "zero-weight channel: not the segment's first row"
    # arg is the original row of the position
    if case.perm32 is None:
        assert torch.equal(o.arg, o.argpos)
    else:
        want = torch.where(ap < n_rows, case.perm32.long()[ap.clamp(0, n_rows - 1)], torch.full_like(ap, n_rows))
        assert torch.equal(o.arg.long(), want)
    # out = leaky(fma(raw - am, scale, bias)) of the call's own raw and tables: the f64 evaluation
    # rounded once is within one f32 ulp of the f32 fma (double rounding)
    g = pb.seg_graph if pb.seg_graph is not None else torch.zeros(S, dtype=torch.long, device=dev)
    d32 = o.raw - o.am[g]                                                      # the kernel's f32 difference
    v = (d32.to(R.D) * o.scale[g].to(R.D) + pb.gn_bias.to(R.D)).float()
    ok = torch.zeros(S, N, dtype=torch.bool, device=dev)
    for cand in (v, torch.nextafter(v, torch.full_like(v, float("inf"))),
                 torch.nextafter(v, torch.full_like(v, float("-inf")))):
        ok |= o.out == torch.where(cand > 0, cand, cand * pb.slope)
    assert bool(ok[live].all()), f"{int((~ok & live).sum())} elements of out are not y(raw) to one ulp"
    del ok, v, d32
    # duplicated rows: where one of them is the arg, it is the first one
    d0 = int(rp[case.dup_seg]) + DUP_AT
    apd = ap[case.dup_seg]
    hit = (apd >= d0) & (apd < d0 + DUP_ROWS) & ~zero_w
    assert bool((apd[hit] == d0).all()), "among bitwise equal rows the first one has to win"

    # ---- bounds ----------------------------------------------------------------------------------
    if parent is not None:
        E = factor * parent["raw"]                          # in units of max |h|
        # the kernel prefers row a to the true winner b only if its own h(a) >= h(b), and each is
        # within E of h64: the reference's extremum is not more than 2 E above h64 at the witness
        assert deficit <= 2 * E, f"witness: {deficit:.3e} of max|h| below the extremum (2 E = {2 * E:.3e})"
        # ... hence, where the equal rows lead every other row by more than 2 E, the first of them
        pos = torch.arange(int(rp[case.dup_seg]), int(rp[case.dup_seg + 1]), device=dev)
        hs = pb.h_at(pos) * sgn
        isd = (pos >= d0) & (pos < d0 + DUP_ROWS)
        lead = hs[isd].max(0).values - hs[~isd].max(0).values
        sure = (lead > 2 * E * st.h_absmax) & ~zero_w
        assert int(sure.sum()) >= 10, "fixture: the equal rows were meant to win in many channels"
        assert bool((apd[sure] == d0).all()), "among bitwise equal rows the first one has to win"
        for q in QUANTITIES:
            assert errs[q] <= factor * parent[q], \
                f"{label} {q}: error {errs[q]:.3e} against the parent's {parent[q]:.3e} (allowed: x {factor:g})"
    if subset is not None:
        sub = R.pool_segments(pb, st, subset, witness=o.argpos[subset], chunk=1 << 18)
        lv = live[subset]
        for f in ("raw", "out", "ext", "h_witness"):         # (a product in other blocks: the last bits may differ)
            d = (getattr(sub, f) - getattr(ref, f)[subset])[lv].abs().max()
            assert float(d) <= 1e-12 * st.h_absmax, f
        assert bool((sub.argpos[~lv] == n_rows).all()) and bool((sub.out[~lv] == 0).all())
        e_raw = float((o.raw[subset].to(R.D) - sub.h_witness)[live[subset]].abs().max()) / st.h_absmax
        assert e_raw <= errs["raw"]
    return errs, st, ref


# ---- backward ----------------------------------------------------------------------------------------
@dataclass
class Grads:
    status: int
    gm: torch.Tensor
    gx: torch.Tensor
    gW: torch.Tensor
    ptot: torch.Tensor


def call_backward(case, mode, o, gout, c1, c2, c3):
    """spt_fused_linear_bwd_pool_runs_f32 on the forward outputs `o`; outputs pre-filled with NaN."""
    pb, S, K, N = case.pb, case.num_seg, case.K, case.N
    dev, B = pb.x.device, pb.num_graphs
    assert (pb.x.dtype == torch.bfloat16) == bool(mode & X_BF16)
    assert gout.shape == (S, N) and c1.shape == c2.shape == c3.shape == (B, N)
    nan = float("nan")
    gm = torch.full((S, N), nan, device=dev)
    gx = torch.full((pb.n_rows, K), nan, device=dev)
    gW = torch.full((N, K), nan, device=dev)
    ptot = torch.full((B, 2 * K + 1), nan, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib.spt_fused_linear_pool_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    n = len(pb.runs)
    r0 = (ctypes.c_int64 * n)(*[r[0] for r in pb.runs])
    r1 = (ctypes.c_int64 * n)(*[r[1] for r in pb.runs])
    rg = (ctypes.c_int32 * n)(*[r[2] for r in pb.runs])
    P = _lib.ptr
    st = _lib.lib.spt_fused_linear_bwd_pool_runs_f32(
        P(gout), P(o.raw), P(o.argpos), P(case.perm32), P(case.pos_seg), P(pb.seg_graph), S, n, r0, r1, rg, B,
        N, P(o.am), P(o.scale), P(pb.gn_bias), pb.slope, P(c1), P(c2), P(c3), P(pb.x), K, P(pb.pre_am),
        P(pb.pre_scale), P(pb.pre_bias), pb.pre_slope, P(pb.W), P(o.gram), P(gm), P(gx), P(gW), P(ptot), mode,
        P(ws), ws.numel(), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return Grads(st, gm, gx, gW, ptot)


def backward_errors(case, o, gr, c2, c3, chunk=1 << 20):
    """Identity (iii) of csrc/fused_pool.hip in f64, in chunks of CSR positions, from the call's own
    inputs (the forward's raw / argpos / Gram record and the gm rows the call's first kernel wrote) -
    the reference of tests/test_fpool_bwd_level_gpu.py, whose error definition
    (max |out - ref| / max |ref| of gx, gW, sum g', sum g' o') this returns:
        gy_i = S_i W + y_i (W^T diag(B) W) + A W,   gW = S^T y + diag(B) W G + A (x) sum_i y_i,
        B = -c2, A = c2 am - c3, S_i[c] = gm[s, c] where position i is the winner of (s, c), else 0;
        g' = gy times the previous activation's slope, o' = x - am_prev."""
    pb, S, K, N = case.pb, case.num_seg, case.K, case.N
    dev, B = pb.x.device, pb.num_graphs
    _lib.check(gr.status, "spt_fused_linear_bwd_pool_runs_f32")
    W = pb.W.to(R.D)
    ap = o.argpos.long().reshape(-1)
    order = torch.argsort(ap)                                # winners by position: a chunk is a slice
    aps = ap[order]
    gms = gr.gm.to(R.D).reshape(-1)[order]
    col = (order % N)
    del order
    gW_ref = torch.zeros(N, K, dtype=R.D, device=dev)
    p1 = torch.zeros(B, K, dtype=R.D, device=dev)
    p2 = torch.zeros(B, K, dtype=R.D, device=dev)
    gx_err, gx_max = 0.0, 0.0
    perm = None if pb.perm is None else pb.perm.long()
    for q0, q1, b in pb.runs:
        Bc = -c2[b].to(R.D)
        Ac = c2[b].to(R.D) * o.am[b].to(R.D) - c3[b].to(R.D)
        M = W.t() @ (Bc[:, None] * W)
        G = o.gram[b, :K * K].view(K, K)
        sy = o.gram[b, K * K:K * K + K]
        gW_ref += Bc[:, None] * (W @ G) + Ac[:, None] * sy[None, :]
        for a in range(q0, q1, chunk):
            e = min(a + chunk, q1)
            pos = torch.arange(a, e, device=dev)
            rows = pos if perm is None else perm[pos]
            ox = pb.x[rows].to(R.D) - pb.pre_am[b].to(R.D)
            yv = ox * pb.pre_scale[b].to(R.D) + pb.pre_bias.to(R.D)
            y = R.leaky(yv, pb.pre_slope)
            lo, hi = torch.searchsorted(aps, torch.tensor([a, e], device=dev)).tolist()
            Sm = torch.zeros(e - a, N, dtype=R.D, device=dev)
            Sm[aps[lo:hi] - a, col[lo:hi]] = gms[lo:hi]
            gy = Sm @ W + y @ M + (Ac @ W)[None, :]
            gW_ref += Sm.t() @ y
            gp = gy * torch.where(yv > 0, 1.0, pb.pre_slope)
            p1[b] += gp.sum(0)
            p2[b] += (gp * ox).sum(0)
            gx_err = _nanmax(gx_err, float((gr.gx[rows].to(R.D) - gy).abs().max()))
            gx_max = max(gx_max, float(gy.abs().max()))
            del Sm, gy, gp, y, yv, ox
    errs = (gx_err / gx_max, _rel(gr.gW, gW_ref),
            _nanmax(*[_rel(gr.ptot[b, :K], p1[b]) for b in range(B)]),
            _nanmax(*[_rel(gr.ptot[b, K:2 * K], p2[b]) for b in range(B)]))
    counts = [gr.ptot[b, 2 * K].item() for b in range(B)]
    return errs, counts
