"""The pool-fused top layer's backward (`spt_fused_linear_bwd_pool_runs_f32`, main kernel
`fpool::bwd_pool_kernel` of csrc/fused_pool.hip) at a size where every workgroup walks many tiles:
3 M rows, ~35 rows per segment, K = 64 -> N = 128 - the largest this layer sees in the suite - in the
f32 mode and in the bf16 mode, with the rows shuffled and in CSR order.

Reference: identity (iii) of the file's header evaluated in float64 from the call's own inputs
(the forward's raw / argpos / Gram record, the `gm` rows the call's first kernel writes):
    gy_i = S_i W + y_prev_i (W^T diag(B) W) + A W,   gW = S^T y_prev + diag(B) W G + A (x) sum_i y_prev_i
    with B = -c2, A = c2 am - c3, S_i[c] = gm[s, c] where row i is the winner of (s, c), else 0,
and the two sums of the previous norm's backward, sum_i g'_i and sum_i g'_i o_i (o = x - am_prev,
g' = gy times the previous activation's slope).

Error per output = max |out - ref| / max |ref|.  The kernel sums in f32 (split-bf16 products in the
f32 mode, plain bf16 operands in the bf16 mode), so the bound is the error of the kernel BEFORE its
tile staging was shared between the waves of a pair (commit aa12fea, measured with this very test
on one MI355X), times two: a change of summation order alone must not move the error by more.

    mode  order      gx        gW        sum g'    sum g' o'
    f32   shuffled   1.151e-05 5.449e-08 2.051e-06 2.663e-06
    f32   csr        1.234e-05 7.553e-08 2.374e-06 2.686e-06
    bf16  shuffled   3.835e-03 1.214e-03 1.326e-03 1.655e-03
    bf16  csr        4.144e-03 8.736e-04 1.516e-03 1.919e-03
"""
import ctypes

import pytest
import torch

from superpoint_transformer_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

ROWS, SEGS, K, N = 3_000_000, 3_000_000 // 35, 64, 128
SLOPE = 0.01

# max |out - ref| / max |ref| of the parent commit's library: (gx, gW, sum g', sum g' o')
PARENT_ERR = {
    (1, "shuffled"): (1.151e-05, 5.449e-08, 2.051e-06, 2.663e-06),
    (1, "csr"): (1.234e-05, 7.553e-08, 2.374e-06, 2.686e-06),
    (3, "shuffled"): (3.835e-03, 1.214e-03, 1.326e-03, 1.655e-03),
    (3, "csr"): (4.144e-03, 8.736e-04, 1.516e-03, 1.919e-03),
}


def _leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


@pytest.mark.parametrize("order", ["shuffled", "csr"])
@pytest.mark.parametrize("mode", [1, 3], ids=["f32", "bf16"])
def test_backward_at_level_size_matches_the_f64_identity(mode, order):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    sizes = synthetic._segment_sizes(g, ROWS, SEGS, "lognormal", dev)
    si = torch.repeat_interleave(torch.arange(SEGS, device=dev), sizes)
    if order == "shuffled":
        si = si[torch.randperm(ROWS, generator=g, device=dev)]
    perm = torch.argsort(si, stable=True).int()
    pos_seg = si[perm.long()].int()
    rowptr = torch.zeros(SEGS + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(si, minlength=SEGS), 0).int()
    x = torch.randn(ROWS, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.1
    gnw = torch.randn(N, device=dev, generator=g)
    gnb, gms = torch.randn(N, device=dev, generator=g) * 0.1, torch.rand(N, device=dev, generator=g)
    pam = torch.randn(1, K, device=dev, generator=g) * 0.1
    psc = torch.rand(1, K, device=dev, generator=g) + 0.5
    pbs = torch.randn(K, device=dev, generator=g) * 0.1
    out, raw = torch.empty(SEGS, N, device=dev), torch.empty(SEGS, N, device=dev)
    arg, argpos = (torch.empty(SEGS, N, dtype=torch.int32, device=dev) for _ in range(2))
    glen = int(_lib.lib.spt_fused_linear_pool_gram_len(K))
    gram = torch.empty(1, glen, dtype=torch.float64, device=dev)
    mean, rstd, am, sc = (torch.empty(1, N, device=dev) for _ in range(4))
    ws = torch.empty(_lib.lib.spt_fused_linear_pool_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    r0, r1, g0 = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(ROWS), (ctypes.c_int32 * 1)(0)
    gout = torch.randn(SEGS, N, device=dev, generator=g)
    c1, c2, c3 = (torch.rand(1, N, device=dev, generator=g) * 0.1 for _ in range(3))
    gm = torch.empty(SEGS, N, device=dev)
    gx = torch.full((ROWS, K), float("nan"), device=dev)
    gW = torch.full((N, K), float("nan"), device=dev)
    ptot = torch.full((1, 2 * K + 1), float("nan"), dtype=torch.float64, device=dev)
    P, sp = _lib.ptr, _lib.stream_ptr(dev)
    assert _lib.lib.spt_fused_linear_pool_supported(K, N, mode)
    _lib.check(_lib.lib.spt_fused_linear_fwd_pool_runs_f32(
        P(x), P(perm), P(pos_seg), P(rowptr), None, SEGS, ROWS, 1, r0, r1, g0, 1, K, P(W), N, P(gnw), P(gnb),
        P(gms), 1e-5, SLOPE, P(pam), P(psc), P(pbs), SLOPE, P(out), P(arg), P(argpos), P(raw), P(gram), None,
        P(mean), P(rstd), P(am), P(sc), mode, P(ws), ws.numel(), sp), "fwd_pool")
    _lib.check(_lib.lib.spt_fused_linear_bwd_pool_runs_f32(
        P(gout), P(raw), P(argpos), P(perm), P(pos_seg), None, SEGS, 1, r0, r1, g0, 1, N, P(am), P(sc), P(gnb),
        SLOPE, P(c1), P(c2), P(c3), P(x), K, P(pam), P(psc), P(pbs), SLOPE, P(W), P(gram), P(gm), P(gx),
        P(gW), P(ptot), mode, P(ws), ws.numel(), sp), "bwd_pool")
    torch.cuda.synchronize()

    # ---- identity (iii) in float64, rows in CSR order ----------------------------------------------
    d = torch.float64
    W64 = W.to(d)
    Bc = -c2[0].to(d)
    Ac = c2[0].to(d) * am[0].to(d) - c3[0].to(d)
    o = x[perm.long()].to(d) - pam.to(d)
    yv = o * psc.to(d) + pbs.to(d)
    pos_slope = torch.where(yv > 0, torch.ones_like(yv), torch.full_like(yv, SLOPE))
    y = _leaky(yv, SLOPE)
    del yv
    S = torch.zeros(ROWS, N, dtype=d, device=dev)
    ap = argpos.long()
    ok = (ap >= 0) & (ap < ROWS)
    cols = torch.arange(N, device=dev).expand(SEGS, N)
    S[ap[ok], cols[ok]] = gm.to(d)[ok]
    M = W64.t() @ (Bc[:, None] * W64)
    gy = S @ W64 + y @ M + (Ac @ W64)[None, :]
    G = gram[0, :K * K].view(K, K)
    sy = gram[0, K * K:K * K + K]
    gW_ref = S.t() @ y + Bc[:, None] * (W64 @ G) + Ac[:, None] * sy[None, :]
    del S
    gx_ref = torch.empty(ROWS, K, dtype=d, device=dev)
    gx_ref[perm.long()] = gy
    gp = gy * pos_slope
    p1_ref, p2_ref = gp.sum(0), (gp * o).sum(0)

    def rel(a, r):
        return ((a.to(d) - r).abs().max() / r.abs().max()).item()

    errs = (rel(gx, gx_ref), rel(gW, gW_ref), rel(ptot[0, :K], p1_ref), rel(ptot[0, K:2 * K], p2_ref))
    print(f"fpool bwd level mode={mode} order={order}: gx {errs[0]:.3e} gW {errs[1]:.3e} "
          f"sum g' {errs[2]:.3e} sum g'o' {errs[3]:.3e}")
    assert ptot[0, 2 * K].item() == ROWS
    assert all(e == e for e in errs), f"NaN in an output: {errs}"
    bound = PARENT_ERR[(mode, order)]
    for name, e, b in zip(("gx", "gW", "sum g'", "sum g' o'"), errs, bound):
        assert e <= 2 * b, f"{name}: error {e:.3e} against the parent's {b:.3e} (allowed: twice that)"
