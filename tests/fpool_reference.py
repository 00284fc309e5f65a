"""Float64 reference of the pool-fused top layer's FORWARD (csrc/fused_pool.hip, entry
spt_fused_linear_fwd_pool_runs_f32), evaluated from the call's own inputs in plain torch on
whatever device the inputs live on.  What it states is the header of fused_pool.hip:

    y   = leaky((x - pre_am[g]) * pre_scale[g] + pre_bias)          (the layer's activated input)
    h   = y W^T                                                      (bf16 mode: of bf16(y), bf16(W))
    per graph: G = sum y y^T, sum y, rows; sum h, sum h^2; mean / rstd / am / scale of the norm
    per (segment, channel): the extremum of h (max for norm weight >= 0, min for < 0), the first
    CSR position attaining it (weight == 0: the segment's first position), 0 / n_rows for an empty
    segment; out = leaky(scale * (raw - am) + bias).

Everything that walks rows does so in chunks of CSR positions (`chunk` rows of f64 work at a
time), so that the statistics can be accumulated over 15 M rows and the per-segment part be asked
for a subset of whole segments only.  tests/test_fpool_reference_cpu.py pins this module on
oracle.spt_model.mlp -> oracle.spt_oracle.scatter_max; the GPU tests compare the kernels with it.
"""
from dataclasses import dataclass

import torch

D = torch.float64


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def round_bf16(t):
    """Round-to-nearest-even to bf16 (from the f32 value, as `(__bf16)` of a float does)."""
    return t.to(torch.float32).to(torch.bfloat16).to(D)


@dataclass
class Problem:
    """The forward call's inputs.  x [n_rows, K] (f32, or bf16 for bf16 storage); perm [n_rows]
    or None (rows already in CSR order); rowptr [num_seg + 1]; runs: list of (p0, p1, graph) CSR
    position ranges; seg_graph [num_seg] or None; W [N, K]; pre_am / pre_scale [B, K], pre_bias [K];
    gn_weight / gn_bias / gn_mean_scale [N]; bf16: the mode rounds y and W to bf16."""
    x: torch.Tensor
    perm: torch.Tensor
    rowptr: torch.Tensor
    runs: list
    seg_graph: torch.Tensor
    W: torch.Tensor
    pre_am: torch.Tensor
    pre_scale: torch.Tensor
    pre_bias: torch.Tensor
    pre_slope: float
    gn_weight: torch.Tensor
    gn_bias: torch.Tensor
    gn_mean_scale: torch.Tensor
    eps: float
    slope: float
    bf16: bool = False

    @property
    def n_rows(self):
        return self.x.shape[0]

    @property
    def num_graphs(self):
        return self.pre_am.shape[0]

    def weight(self):
        return round_bf16(self.W) if self.bf16 else self.W.to(D)

    def graph_of_positions(self, pos):
        g = torch.zeros_like(pos)
        for p0, p1, b in self.runs:
            g = torch.where((pos >= p0) & (pos < p1), torch.full_like(pos, b), g)
        return g

    def y_at(self, pos):
        """The activated input (f64) of the rows at CSR positions `pos` (int64)."""
        rows = pos if self.perm is None else self.perm.long()[pos]
        g = self.graph_of_positions(pos)
        v = (self.x[rows].to(D) - self.pre_am.to(D)[g]) * self.pre_scale.to(D)[g] + self.pre_bias.to(D)
        y = leaky(v, self.pre_slope)
        return round_bf16(y) if self.bf16 else y

    def h_at(self, pos):
        return self.y_at(pos) @ self.weight().t()


@dataclass
class Stats:
    gram: torch.Tensor        # [B, K K + K + 1]: G | sum y | rows
    total: torch.Tensor       # [B, 2 N + 1]: sum h | sum h^2 | rows
    mean: torch.Tensor        # [B, N] each
    rstd: torch.Tensor
    am: torch.Tensor
    scale: torch.Tensor
    h_absmax: float           # max |h| over all rows


def statistics(pb, chunk=1 << 20):
    """Per-graph sums over the rows, accumulated chunk by chunk, and the norm's tables by the
    formulas of oracle.spt_oracle.graph_norm:  mean = sum h / n;  the centred value is
    h - mean_scale * mean, so  var = E[h^2] - (2 a - a^2) mean^2;  rstd = 1 / sqrt(var + eps);
    am = a * mean;  scale = weight * rstd."""
    dev = pb.x.device
    K, N, B = pb.W.shape[1], pb.W.shape[0], pb.num_graphs
    gram = torch.zeros(B, K * K + K + 1, dtype=D, device=dev)
    total = torch.zeros(B, 2 * N + 1, dtype=D, device=dev)
    W = pb.weight()
    hmax = 0.0
    for p0, p1, b in pb.runs:
        for a in range(p0, p1, chunk):
            pos = torch.arange(a, min(a + chunk, p1), device=dev)
            y = pb.y_at(pos)
            h = y @ W.t()
            gram[b, :K * K] += (y.t() @ y).reshape(-1)
            gram[b, K * K:K * K + K] += y.sum(0)
            gram[b, K * K + K] += pos.numel()
            total[b, :N] += h.sum(0)
            total[b, N:2 * N] += (h * h).sum(0)
            total[b, 2 * N] += pos.numel()
            hmax = max(hmax, float(h.abs().max()))
            del y, h
    n = total[:, 2 * N].clamp(min=1.0)[:, None]
    a = pb.gn_mean_scale.to(D)[None, :]
    mean = total[:, :N] / n
    var = (total[:, N:2 * N] / n - (2 * a - a * a) * mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + pb.eps)
    return Stats(gram, total, mean, rstd, a * mean, pb.gn_weight.to(D)[None, :] * rstd, hmax)


@dataclass
class Pooled:
    raw: torch.Tensor         # [S, N] f64: h of the winner (0 for an empty segment)
    argpos: torch.Tensor      # [S, N] int64: first CSR position attaining the extremum (n_rows: empty)
    out: torch.Tensor         # [S, N] f64
    ext: torch.Tensor         # [S, N] f64: sgn * raw, the maximum of sgn * h (-inf: empty)
    h_witness: torch.Tensor   # [S, N] f64 or None: h at the caller's positions (NaN outside the segment)


def _pool_block(pb, st, segs, witness):
    dev = pb.x.device
    N, S = pb.W.shape[0], segs.numel()
    rp = pb.rowptr.long()
    a0, a1 = rp[segs], rp[segs + 1]
    cnt = a1 - a0
    loc = torch.repeat_interleave(torch.arange(S, device=dev), cnt)          # local segment of a row
    first = torch.cumsum(cnt, 0) - cnt                                       # local offset of a segment
    pos = a0[loc] + (torch.arange(loc.numel(), device=dev) - first[loc])     # its CSR position
    h = pb.h_at(pos)
    w = pb.gn_weight
    sgn = torch.where(w < 0, -1.0, 1.0).to(D)
    hs = h * sgn
    idx = loc[:, None].expand(-1, N)
    ext = torch.full((S, N), float("-inf"), dtype=D, device=dev)
    ext.scatter_reduce_(0, idx, hs, "amax", include_self=True)
    cand = torch.where(hs == ext[loc], pos[:, None].expand(-1, N), torch.full_like(idx, pb.n_rows))
    argpos = torch.full((S, N), pb.n_rows, dtype=torch.int64, device=dev)
    argpos.scatter_reduce_(0, idx, cand, "amin", include_self=True)
    del cand
    empty = cnt == 0
    zero = (w == 0)[None, :] & ~empty[:, None]                               # every row ties: the first
    argpos = torch.where(zero, a0[:, None].expand(-1, N), argpos)
    # h of the winner: its local row is argpos - a0 + first
    lrow = (argpos - a0[:, None] + first[:, None]).clamp(0, max(loc.numel() - 1, 0))
    if loc.numel():
        raw = torch.where(empty[:, None], torch.zeros((), dtype=D, device=dev), h.gather(0, lrow))
    else:
        raw = torch.zeros(S, N, dtype=D, device=dev)
    ext = torch.where(zero, raw * sgn, ext)
    g = pb.seg_graph.long()[segs] if pb.seg_graph is not None else torch.zeros_like(segs)
    out = leaky(st.scale[g] * (raw - st.am[g]) + pb.gn_bias.to(D), pb.slope)
    out = torch.where(empty[:, None], torch.zeros((), dtype=D, device=dev), out)
    hw = None
    if witness is not None:
        wp = witness.long()
        inside = (wp >= a0[:, None]) & (wp < a1[:, None])
        if loc.numel():
            lw = (wp - a0[:, None] + first[:, None]).clamp(0, loc.numel() - 1)
            hw = torch.where(inside, h.gather(0, lw), torch.full((), float("nan"), dtype=D, device=dev))
        else:
            hw = torch.full((S, N), float("nan"), dtype=D, device=dev)
    return raw, argpos, out, ext, hw


def pool_segments(pb, st, segs, witness=None, chunk=1 << 20):
    """The per-segment part on the whole segments `segs` (int64 ids, any order, any subset), in
    blocks of about `chunk` rows.  `witness` [len(segs), N]: CSR positions (the kernel's argpos)
    at which h is reported too."""
    dev = pb.x.device
    segs = segs.to(dev).long()
    rp = pb.rowptr.long()
    csum = torch.cumsum(rp[segs + 1] - rp[segs], 0).cpu()
    parts, lo = [], 0
    while lo < segs.numel():
        base = int(csum[lo - 1]) if lo else 0
        hi = int(torch.searchsorted(csum, torch.tensor(base + chunk), right=True))
        hi = min(max(hi, lo + 1), segs.numel())
        parts.append(_pool_block(pb, st, segs[lo:hi], None if witness is None else witness[lo:hi]))
        lo = hi
    if not parts:
        parts = [_pool_block(pb, st, segs, witness)]
    cat = [torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None for i in range(5)]
    return Pooled(*cat)
