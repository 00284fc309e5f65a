"""One-pass backward of the attention blocks' Linears (csrc/skinny_linear.hip:
`spt_skinny_linear_bwd_m_f32`): gx, gW and gb from one read of gy and x.

The C entry is called directly (the autograd wrappers route >= 4096 rows only):
  gx  bitwise `spt_skinny_linear_wt_m_f32` (the two-launch route's input gradient, same mode);
  gW, gb  against an f64 product of the same operands, max |diff| < 2e-5 max |ref| (the bar of
      tests/test_prenorm_fused_gpu.py::test_linear_residual_and_norm_linear_against_f64); the bf16
      mode against the f64 product of the bf16-ROUNDED operands at 2^-8 sqrt(rows) of the product
      scale (tests/test_skinny_linear_gpu.py::test_matrix_modes_of_the_skinny_linears' bar for that
      mode, the contraction here being the rows); gb sums unrounded values in both modes;
  the error of today's `spt_skinny_dw_pre_m_f32` against the same reference is printed next to it;
  PRE (1 and 3 graphs) bitwise the plain instance on rows normalised by `spt_graphnorm_apply_f32`;
  run twice: same bits; exact-size guarded workspace: same bits, guards intact; one byte short: refused.
"""
import functools

import pytest
import torch

from guarded import GuardedArena

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 17, 63, 64, 65, 16 * 131 + 5, 4096 + 5, 16 * 4200 + 3]
SHAPES = [(64, 192), (64, 64)]
MODES = [1, 3]                                           # split bf16 (the default), bf16


def L():
    from superpoint_transformer_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def inputs(rows, K, N):
    """Seeded operands and their f64 products, made once per (rows, K, N)."""
    g = torch.Generator().manual_seed(rows * 7 + K + N)
    gy, x = torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.1
    ref = {1: (gy.double().t() @ x.double(), gy.double().sum(0))}
    rb = lambda t: t.bfloat16().double()
    ref[3] = (rb(gy).t() @ rb(x), ref[1][1])
    return gy, x, W, ref


def fused(dev, gy, x, W, mode, pre=None, ws=None, ws_bytes=None, want_gb=True):
    lb = L()
    rows, K = x.shape
    N = gy.shape[1]
    gx = torch.full((rows, K), float("nan"), device=dev)
    gw = torch.full((N, K), float("nan"), device=dev)
    gb = torch.full((N,), float("nan"), device=dev) if want_gb else None
    if ws is None:
        ws = torch.empty(lb.lib.spt_skinny_linear_bwd_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    am, sc, pb, batch, B = pre if pre is not None else (None, None, None, None, 1)
    with torch.cuda.device(dev):
        st = lb.lib.spt_skinny_linear_bwd_m_f32(
            lb.ptr(gy), lb.ptr(x), lb.ptr(W), rows, N, K, lb.ptr(gx), lb.ptr(gw), lb.ptr(gb), lb.ptr(am),
            lb.ptr(sc), lb.ptr(pb), lb.ptr(batch), B, mode, lb.ptr(ws),
            ws.numel() if ws_bytes is None else ws_bytes, lb.stream_ptr(dev))
    return st, gx, gw, gb


def two_launch(dev, gy, x, W, mode):
    lb = L()
    rows, K = x.shape
    N = gy.shape[1]
    gx = torch.empty((rows, K), device=dev)
    gw, gb = torch.empty((N, K), device=dev), torch.empty(N, device=dev)
    ws = torch.empty(lb.lib.spt_skinny_dw_workspace_bytes(K, N), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lb.check(lb.lib.spt_skinny_linear_wt_m_f32(lb.ptr(gy), rows, N, lb.ptr(W), K, lb.ptr(gx), mode,
                                                   lb.stream_ptr(dev)), "spt_skinny_linear_wt_m_f32")
        lb.check(lb.lib.spt_skinny_dw_pre_m_f32(lb.ptr(gy), lb.ptr(x), rows, N, K, lb.ptr(gw), lb.ptr(gb),
                                                None, None, None, None, 1, mode, lb.ptr(ws), ws.numel(),
                                                lb.stream_ptr(dev)), "spt_skinny_dw_pre_m_f32")
    return gx, gw, gb


def bars(rows, gy, x, ref, mode):
    rw, rb = ref[mode]
    if mode == 3:
        return 2.0 ** -8 * max(rows, 1) ** 0.5 * float(gy.abs().max()) * float(x.abs().max()), \
            2e-5 * float(rb.abs().max())
    return 2e-5 * float(rw.abs().max()), 2e-5 * float(rb.abs().max())


@pytest.mark.parametrize("mode", MODES, ids=["split-bf16", "bf16"])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_one_pass_backward(rows, K, N, mode, dev):
    lb = L()
    assert lb.lib.spt_skinny_linear_bwd_supported(K, N, 1, mode)
    gy, x, W, ref = inputs(rows, K, N)
    dgy, dx, dW = gy.to(dev), x.to(dev), W.to(dev)
    st, gx, gw, gb = fused(dev, dgy, dx, dW, mode)
    lb.check(st, "spt_skinny_linear_bwd_m_f32")
    assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all()
    ox, ow, ob = two_launch(dev, dgy, dx, dW, mode)
    assert torch.equal(gx, ox), "gx differs from spt_skinny_linear_wt_m_f32"
    rw, rb = ref[mode]
    ew, eb = (gw.cpu().double() - rw).abs().max().item(), (gb.cpu().double() - rb).abs().max().item()
    ow_, ob_ = (ow.cpu().double() - rw).abs().max().item(), (ob.cpu().double() - rb).abs().max().item()
    bw, bb = bars(rows, gy, x, ref, mode)
    print(f"rows={rows} K={K} N={N} mode={mode}: gW err one-pass {ew:.3e} two-launch {ow_:.3e} bar {bw:.3e} | "
          f"gb err one-pass {eb:.3e} two-launch {ob_:.3e} bar {bb:.3e}")
    assert ew < bw and eb < bb
    # a second run: same bits
    st, gx2, gw2, gb2 = fused(dev, dgy, dx, dW, mode)
    lb.check(st, "spt_skinny_linear_bwd_m_f32")
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # gb is optional and changes nothing else
    st, gx3, gw3, gb3 = fused(dev, dgy, dx, dW, mode, want_gb=False)
    lb.check(st, "spt_skinny_linear_bwd_m_f32")
    assert gb3 is None and torch.equal(gx, gx3) and torch.equal(gw, gw3)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("rows", [65, 16 * 131 + 5, 4096 + 5])
def test_prenorm_instance_is_bitwise_the_plain_one_on_normalised_rows(rows, K, N, B, dev):
    lb = L()
    gy, x, W, _ = inputs(rows, K, N)
    g = torch.Generator().manual_seed(B + rows)
    am = torch.randn(B, K, generator=g).to(dev)
    sc = (torch.rand(B, K, generator=g) + 0.5).to(dev)
    pb = torch.randn(K, generator=g).to(dev)
    batch = (torch.arange(rows) * B // rows).to(dev)             # sorted graph ids
    dgy, dx, dW = gy.to(dev), x.to(dev), W.to(dev)
    xn = torch.empty_like(dx)
    with torch.cuda.device(dev):
        lb.check(lb.lib.spt_graphnorm_apply_f32(lb.ptr(dx), lb.ptr(batch), rows, K, B, lb.ptr(am), lb.ptr(sc),
                                                lb.ptr(pb), 1.0, lb.ptr(xn), lb.stream_ptr(dev)),
                 "spt_graphnorm_apply_f32")
    for mode in MODES:
        assert lb.lib.spt_skinny_linear_bwd_supported(K, N, B, mode)
        st, gx1, gw1, gb1 = fused(dev, dgy, dx, dW, mode, pre=(am, sc, pb, batch if B > 1 else None, B))
        lb.check(st, "spt_skinny_linear_bwd_m_f32 (pre)")
        st, gx0, gw0, gb0 = fused(dev, dgy, xn, dW, mode)
        lb.check(st, "spt_skinny_linear_bwd_m_f32")
        assert torch.equal(gw1, gw0) and torch.equal(gb1, gb0)
        assert torch.equal(gx1, gx0)                             # gx does not see x at all
    # too many graphs for the tables in LDS
    assert not lb.lib.spt_skinny_linear_bwd_supported(K, N, 1024 // K + 1, 1)


def test_shapes_and_modes_that_keep_the_two_launch_route():
    lb = L().lib
    assert lb.spt_skinny_linear_bwd_supported(64, 192, 16, 1) and lb.spt_skinny_linear_bwd_supported(64, 64, 1, 3)
    assert not lb.spt_skinny_linear_bwd_supported(64, 192, 17, 1)        # tables past the LDS cap
    assert not lb.spt_skinny_linear_bwd_supported(64, 192, 1, 0)         # the f32-exact mode
    assert not lb.spt_skinny_linear_bwd_supported(128, 384, 1, 1) and not lb.spt_skinny_linear_bwd_supported(192, 64, 1, 1)
    assert not lb.spt_skinny_linear_bwd_supported(64, 13, 1, 1) and not lb.spt_skinny_linear_bwd_supported(64, 128, 1, 1)


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("rows", [65, 16 * 4200 + 3])
def test_exact_workspace_and_short_workspace(rows, K, N, dev):
    lb = L()
    gy, x, W, _ = inputs(rows, K, N)
    dgy, dx, dW = gy.to(dev), x.to(dev), W.to(dev)
    st, gx, gw, gb = fused(dev, dgy, dx, dW, 1)
    lb.check(st, "spt_skinny_linear_bwd_m_f32")
    need = lb.lib.spt_skinny_linear_bwd_workspace_bytes(K, N)
    arena = GuardedArena(dev)
    st, gx2, gw2, gb2 = fused(dev, dgy, dx, dW, 1, ws=arena.take(need, label="skinny bwd ws"))
    lb.check(st, "spt_skinny_linear_bwd_m_f32")
    arena.check()
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # one byte short: refused before any launch (the NaN pre-fill stays)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st, gx3, gw3, gb3 = fused(dev, dgy, dx, dW, 1, ws=ws, ws_bytes=need - 1)
    assert st != 0 and "workspace" in lb.last_error()
    torch.cuda.synchronize(dev)
    assert torch.isnan(gx3).all() and torch.isnan(gw3).all() and torch.isnan(gb3).all()


def _ops_case(dev, which, N, fused_on):
    """gx, gW, gb (and for the norm route the norm's own gradients) of one Linear at 5000 rows through
    the autograd classes, with the switch on or off; the route counters' increments."""
    from superpoint_transformer_amd import ops
    rows, K, B = 5000, 64, 3
    g = torch.Generator().manual_seed(N + 11)
    x = (torch.randn(rows, K, generator=g) * 2 + 0.5).to(dev).requires_grad_()
    W = (torch.randn(N, K, generator=g) * 0.1).to(dev).requires_grad_()
    b = (torch.randn(N, generator=g) * 0.1).to(dev).requires_grad_()
    go = torch.randn(rows, N, generator=g).to(dev)
    prev = ops.skinny_bwd_fused(fused_on)
    before = ops.skinny_bwd_route_counts()
    try:
        if which == "tall":
            y = ops.linear(x, W, b)
            grads = torch.autograd.grad(y, (x, W, b), go)
        elif which == "residual":
            res = torch.randn(rows, N, generator=g).to(dev).requires_grad_()
            assert ops.linear_residual_ok(res, W)
            y = ops.linear_residual(x, W, b, res)
            grads = torch.autograd.grad(y, (x, W, b, res), go)
        else:
            batch = (torch.arange(rows) * B // rows).to(dev)
            pw, pb, pa = ((torch.rand(K, generator=g) + 0.5).to(dev).requires_grad_() for _ in range(3))
            assert ops.norm_linear_ok(x, batch, B, W)
            y, xres = ops.norm_linear(x, batch, B, pw, pb, pa, 1e-5, W, b)
            grads = torch.autograd.grad((y * go).sum() + (xres * xres).sum(), (x, W, b, pw, pb, pa))
    finally:
        ops.skinny_bwd_fused(prev)
    after = ops.skinny_bwd_route_counts()
    return [t.detach() for t in grads], {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("N", [192, 64])
@pytest.mark.parametrize("which", ["tall", "residual", "norm"])
def test_autograd_classes_take_the_route_of_the_switch(which, N, dev):
    on, ron = _ops_case(dev, which, N, True)
    off, roff = _ops_case(dev, which, N, False)
    assert ron == {"fused": 1, "split": 0} and roff == {"fused": 0, "split": 1}
    assert torch.equal(on[0], off[0]), "gx"
    for i in (1, 2):                                             # gW, gb: another summation order
        assert (on[i].double() - off[i].double()).abs().max() < 2e-5 * float(off[i].abs().max())
    for a, b_ in zip(on[3:], off[3:]):                           # downstream of gx only
        assert torch.equal(a, b_)
