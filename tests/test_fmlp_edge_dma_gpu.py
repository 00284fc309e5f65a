"""The edge MLP's backward staged by LDS-DMA (csrc/fused_mlp_dma.hip, `bwd_dma_kernel<32, 32, 4, 4>`,
plain and with the 18 -> 32 bottom layer folded into it) against the register-staged
kernels of csrc/fused_mlp.hip (`bwd_kernel_bf<8, 2, ...>`).

The DMA instances run on the register-staged launch's grid with the same tile -> wave mapping, the
same products per tile, one table per workgroup summed wave 1, 2, 3 into wave 0 and per-wave f64
statistics records, so everything they write - gx, gW, the statistics, the fold's raw A | G tables,
gW0 and the norms' parameter gradients - must equal the register-staged route's BIT FOR BIT.  The
outputs therefore cannot tell which route ran: every case asks `spt_fused_linear_bwd_route`.

x0 rows are 72 bytes: a run that starts at an odd row has 8-byte aligned tiles ([1029, 11, 1061]
and [7, 1, 16, 33] below); runs shorter than a tile end in tiles whose DMA must not read past the
run's last row."""
import ctypes

import pytest
import torch

from test_fmlp_bottom_fold_gpu import EPS, SLOPE, _inputs

pytestmark = pytest.mark.gpu

K, N, K0 = 32, 32, 18
MAX_TABS = 1024                                  # FOLD_MAX_TABS of fmlp_bwd_impl's workspace layout
FLEN = (K + 32) * 32                             # A [K][ZP] | G [ZP][ZP], ZP = 32


# 16 * 4200 + 3 rows: 4201 tiles on 1024 workgroups x 4 waves - waves walk several tiles
@pytest.mark.parametrize("rows", [1, 15, 17, 16 * 131 + 5, 16 * 4200 + 3])
def test_plain_32x32_dma_backward_is_bitwise_the_register_staged_one(rows, dev):
    from superpoint_transformer_amd import _lib
    g = torch.Generator().manual_seed(rows + K + N)
    t = lambda *s: torch.randn(*s, generator=g).to(dev)
    h, x, W, gy = t(rows, N), t(rows, K), t(N, K) * 0.1, t(rows, N)
    tabN = [(torch.rand(N, generator=g) + 0.5).to(dev) for _ in range(6)]
    tabK = [(torch.rand(K, generator=g) + 0.5).to(dev) for _ in range(3)]
    ws = torch.empty(_lib.lib.spt_fused_linear_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    P = _lib.ptr

    def run(mode):
        gx = torch.full((rows, K), float("nan"), device=dev)
        gW = torch.empty(N, K, device=dev)
        prev = torch.empty(2 * K + 1, dtype=torch.float64, device=dev)
        st = _lib.lib.spt_fused_linear_bwd_ex_f32(
            P(gy), P(h), 0, rows, N, P(tabN[0]), P(tabN[1]), P(tabN[2]), 0.01, P(tabN[3]),
            P(tabN[4]), P(tabN[5]), P(x), K, P(tabK[0]), P(tabK[1]), P(tabK[2]), 0.2, P(W), P(gx),
            P(gW), 0, P(prev), mode, P(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(st, "fused backward")
        torch.cuda.synchronize()
        return gx, gW, prev

    prev_dma = _lib.lib.spt_fused_linear_bwd_use_dma(1)
    try:
        for p in (1, 3):                                        # split-bf16, bf16
            assert _lib.lib.spt_fused_linear_bwd_route(0, K, N, p) == 1
            assert _lib.lib.spt_fused_linear_bwd_route(0, K, N, p | 4) == 0
            a = run(p)
            b = run(p | 4)                                      # SPT_FMLP_BWD_REGISTER_STAGED
            assert bool(torch.isfinite(a[0]).all()), "a row of gx was not written"
            for name, u, v in zip(("gx", "gW", "statistics"), a, b):
                assert torch.equal(u, v), f"mode {p}: {name} differs from the register-staged route"
    finally:
        _lib.lib.spt_fused_linear_bwd_use_dma(prev_dma)


def _fold_tables(saved, gr, gy, dev):
    """The upper layer's folded backward through the C entry on a zeroed workspace of its own: the
    raw per-workgroup fold tables (the whole table region) and gW0."""
    from superpoint_transformer_amd import _lib, ops
    P = _lib.ptr
    sv = list(saved)
    x2, batch = sv[0], sv[1]
    hs = sv[2:4]
    tabs = [tuple(sv[4 + 4 * i: 8 + 4 * i]) for i in range(2)]
    Ws, gnw, gnb, gms = sv[12:14], sv[14:16], sv[16:18], sv[18:20]
    R, B = x2.shape[0], gr.B
    nr, c_r0, c_r1, c_g = gr.c_arrays()
    sp = _lib.stream_ptr(dev)
    mean, rstd, am, sc = tabs[1]
    total = torch.empty((B, 2 * N + 1), dtype=torch.float64, device=dev)
    w0 = ops._workspace(_lib.lib.spt_graphnorm_workspace_bytes(R, N, B), dev)
    _lib.check(_lib.lib.spt_graphnorm_bwd_stats_f32(
        P(hs[1]), P(gy), P(batch) if B > 1 else None, R, N, B, P(am), P(sc), P(gnb[1]), SLOPE,
        P(total), P(w0), w0.numel(), sp), "spt_graphnorm_bwd_stats_f32")
    c1, c2, c3 = (torch.empty((B, N), device=dev) for _ in range(3))
    gw_n, gb_n, ga_n = (torch.empty(N, device=dev) for _ in range(3))
    _lib.check(_lib.lib.spt_graphnorm_bwd_tables_f32(
        P(total), B, N, P(gnw[1]), P(gms[1]), P(mean), P(rstd), P(c1), P(c2), P(c3), P(gw_n),
        P(gb_n), P(ga_n), sp), "spt_graphnorm_bwd_tables_f32")
    nxt = (*(torch.empty((B, K), device=dev) for _ in range(3)),
           *(torch.empty(K, device=dev) for _ in range(3)))
    pn = _lib.GnBwdTables(P(gnw[0]), P(gms[0]), P(tabs[0][0]), P(tabs[0][1]), *[P(t) for t in nxt])
    ws = torch.zeros(_lib.lib.spt_fused_linear_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    gW = torch.empty((N, K), device=dev)
    gW0 = torch.empty((K, K0), device=dev)
    _lib.check(_lib.lib.spt_fused_linear_bwd_runs_gn_fold_f32(
        P(gy), P(hs[1]), nr, c_r0, c_r1, c_g, B, N, P(am), P(sc), P(gnb[1]), SLOPE, P(c1), P(c2),
        P(c3), P(hs[0]), K, P(tabs[0][2]), P(tabs[0][3]), P(gnb[0]), SLOPE, P(Ws[1]), P(gW), -1,
        P(ws), ws.numel(), ctypes.addressof(pn), P(x2), K0, P(Ws[0]), P(gW0), sp),
        "spt_fused_linear_bwd_runs_gn_fold_f32")
    torch.cuda.synchronize()
    f = ws.view(torch.float32)
    return f[MAX_TABS * N * K: MAX_TABS * (N * K + FLEN)].clone(), gW0


@pytest.mark.parametrize("runs,offset", [
    ([16 * 131 + 5], False),
    ([1029, 11, 1061], False),                   # odd run starts, a run under one tile
    ([7, 1, 16, 33], False),                     # every run shorter than or near a tile, odd starts
    ([16 * 12500 + 5], True),                    # many workgroups' tables meet; the 10 sigma column
])
def test_fold_18x32x32_dma_backward_is_bitwise_the_register_staged_one(runs, offset, dev):
    from superpoint_transformer_amd import _lib, ops
    x, params, gy, batch = _inputs(K0, N, runs, False, offset, dev)
    B, rows = len(runs), sum(runs)
    gr = ops.graph_runs(batch if B > 1 else None, B, rows)
    assert gr is not None and gr.B == B
    _, saved, _, _ = ops._fmlp_forward(x, batch if B > 1 else None, gr, [EPS, EPS], [SLOPE, SLOPE], params)
    meta = (2, gr, [SLOPE, SLOPE], torch.float32, False, -1)

    def backward(dma):
        prev_dma = _lib.lib.spt_fused_linear_bwd_use_dma(dma)
        prev_fold = ops.fold_bottom(True)
        try:
            assert _lib.lib.spt_fused_linear_bwd_route(K0, K, N, -1) == dma, "not the route asked for"
            gx0, grads = ops._fmlp_backward(saved, meta, gy)
            assert gx0 is None
            torch.cuda.synchronize()
            tables, gW0 = _fold_tables(saved, gr, gy, dev)
        finally:
            ops.fold_bottom(prev_fold)
            _lib.lib.spt_fused_linear_bwd_use_dma(prev_dma)
        assert torch.equal(gW0, grads[0]), "the C entry and ops._fmlp_backward disagree on gW0"
        return grads, tables

    (new, tab_new), (old, tab_old) = backward(1), backward(0)
    names = ["gW0", "gn0.weight", "gn0.bias", "gn0.mean_scale", "gW1", "gn1.weight", "gn1.bias", "gn1.mean_scale"]
    for n, a, o in zip(names, new, old):
        assert bool(torch.isfinite(a).all()), f"{n}: not finite"
        assert torch.equal(a, o), f"{n}: differs from the register-staged route"
    assert bool((tab_old != 0).any()), "no fold table was written"
    assert torch.equal(tab_new, tab_old), "raw fold tables differ from the register-staged route"
