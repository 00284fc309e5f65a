"""Both level-0 -> level-1 max-pools at the north-star shape: [15 M, 128] rows into 428 571 segments.
15 M x 128 is 1.92 G elements (89 % of INT32_MAX) and 7.68 GB of f32 (byte offsets beyond 2^32);
the pool-fused route's [15 M, 64] input is 3.84 GB (beyond 2^31 bytes).  Full-tensor properties on
the GPU plus the reference on 300 whole segments drawn with a fixed seed (with the first, the last
and the largest segment and the empty ones among them), as tests/test_fullsize_gpu.py does it for
the norms.

The pool-fused test reuses the harness and the bounds of tests/test_fpool_fwd_level_gpu.py and
tests/test_fpool_bwd_level_gpu.py: the 3 M bound (twice the parent's error there) of the same mode,
shuffled rows, times two - a wave accumulates five times more rows into its f32 statistics, the
per-element product error does not grow with the row count.  Measured at this size with the parent
commit's library (cbc4cef; profiles/r08a_fpool_fwd_level_errors.txt) - it needs no more than that:

    forward  raw       out       G         sum_y     sum_h     sum_h2    mean      rstd      am        scale
    f32      2.973e-07 1.868e-06 2.386e-06 2.940e-08 2.047e-08 1.395e-06 5.029e-08 1.661e-06 6.330e-08 1.830e-06
    bf16     1.112e-03 1.412e-03 9.452e-08 3.155e-08 1.422e-08 4.131e-08 4.490e-08 9.773e-08 5.330e-08 1.085e-07
    backward gx        gW        sum g'    sum g' o'
    f32      1.363e-05 4.423e-08 2.998e-06 3.637e-06
    bf16     4.273e-03 1.210e-03 1.596e-03 2.132e-03
"""
import pytest
import torch

import fpool_harness as H
import test_fpool_bwd_level_gpu as BWD
import test_fpool_fwd_level_gpu as FWD
from oracle import spt_oracle as O
from superpoint_transformer_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

ROWS, C, SEGS, SPOT = 15_000_000, 128, 428_571, 300
CHUNK = 1 << 20


def _spot_segments(sizes, dev):
    """300 segments by a fixed seed, plus the first, the last, the largest and five empty ones."""
    g = torch.Generator().manual_seed(4)
    pick = torch.randint(0, SEGS, (SPOT,), generator=g).to(dev)
    empty = torch.nonzero(sizes == 0).flatten()[:5]
    fixed = torch.tensor([0, SEGS - 1, int(sizes.argmax())], device=dev)
    return torch.unique(torch.cat([pick, fixed, empty]))


def test_standalone_max_pool_at_scene_size(dev):
    """`ops.segment_reduce(max, return_arg=True)` (the row-streaming `segmax_stream_kernel`), its
    backward, and the lane-group formulation of the same forward, on x [15 M, 128] f32 with forced
    ties, lognormal segment sizes, shuffled rows and empty segments.  A max has no rounding: every
    comparison is exact.

    Peak device memory about 18 GB: x 7.68 GB + its gradient 7.68 GB, the index and its CSR view
    0.4 GB, four [428 571, 128] tables 0.9 GB, row chunks of 1 M rows (0.5 GB each) for the
    full-tensor properties.  The gradient is freed before the second formulation runs."""
    from superpoint_transformer_amd import ops
    g = torch.Generator(device=dev).manual_seed(8)
    live = torch.rand(SEGS, generator=g, device=dev) >= 0.01
    live[[0, SEGS - 1]] = False
    live[SEGS // 2] = True
    sizes = torch.zeros(SEGS, dtype=torch.long, device=dev)
    sizes[live] = synthetic._segment_sizes(g, ROWS, int(live.sum()), "lognormal", dev)
    idx = torch.repeat_interleave(torch.arange(SEGS, device=dev), sizes)
    idx = idx[torch.randperm(ROWS, generator=g, device=dev)]
    x = torch.empty(ROWS, C, device=dev)
    for a in range(0, ROWS, CHUNK):                          # few distinct values: ties everywhere
        n = min(CHUNK, ROWS - a)
        v = torch.randint(-4, 5, (n, C), generator=g, device=dev).float()
        v += (torch.rand(n, C, generator=g, device=dev) < 0.3).float() * torch.randn(n, C, generator=g, device=dev)
        x[a:a + n] = v
    del v
    x.requires_grad_()
    mx, arg = ops.segment_reduce(x, idx, SEGS, "max", return_arg=True)
    xd, mxd = x.detach(), mx.detach()
    nonempty = sizes > 0
    assert int((~nonempty).sum()) > 1000
    # sentinel and value of empty segments; arg is a witness inside its own segment
    assert bool((arg[~nonempty] == ROWS).all()) and bool((mxd[~nonempty] == 0).all())
    rows = arg[nonempty].long()
    assert bool(((rows >= 0) & (rows < ROWS)).all())
    assert torch.equal(xd.gather(0, rows), mxd[nonempty])
    assert torch.equal(idx[rows], torch.nonzero(nonempty).expand(-1, C))
    for a in range(0, ROWS, CHUNK):                          # upper bound, everywhere
        assert bool((mxd[idx[a:a + CHUNK]] >= xd[a:a + CHUNK]).all())
    # the oracle on whole segments: values and arg rows (the FIRST row attaining the maximum)
    spot = _spot_segments(sizes, dev)
    member = torch.nonzero(torch.isin(idx, spot)).flatten()              # ascending rows
    local = torch.searchsorted(spot, idx[member])
    ref, rarg = O.scatter_max(xd[member].cpu().double(), local.cpu(), dim_size=spot.numel())
    rarg_rows = torch.where(rarg < member.numel(), member.cpu()[rarg.clamp(max=member.numel() - 1)],
                            torch.full_like(rarg, ROWS))
    assert torch.equal(mxd[spot].cpu().double(), ref)
    assert torch.equal(arg[spot].cpu().long(), rarg_rows)
    # backward: a row belongs to one segment, so it wins at most once per channel and nothing is
    # summed - the gradient is gout[s, c] at (arg[s, c], c) and zero elsewhere
    gout = torch.randn(SEGS, C, generator=g, device=dev)
    gout[gout == 0] = 1.0
    (mx * gout).sum().backward()
    grad = x.grad
    assert torch.equal(grad.gather(0, rows), gout[nonempty])
    assert bool((torch.count_nonzero(grad, dim=0) == int(nonempty.sum())).all())
    x.grad = None
    del grad, gout, rows, mx
    torch.cuda.empty_cache()
    # the lane-group-per-segment formulation of the same forward: bitwise the same
    view = ops.csr_of(idx, SEGS)
    mx0 = torch.full((SEGS, C), float("nan"), device=dev)
    arg0 = torch.full((SEGS, C), -1, dtype=torch.int32, device=dev)
    P = _lib.ptr
    _lib.check(_lib.lib.spt_segcsr_reduce_ex_f32(3, P(xd), P(view.perm), P(view.rowptr), ROWS, SEGS, C, P(mx0),
                                                 P(arg0), 0, _lib.stream_ptr(dev)), "spt_segcsr_reduce_ex_f32")
    torch.cuda.synchronize()
    assert torch.equal(mx0, mxd) and torch.equal(arg0, arg)


@pytest.mark.parametrize("mode", [1, 3], ids=["f32", "bf16"])
def test_pool_fused_top_layer_at_scene_size(mode, dev):
    """Forward and backward C entries of the pool-fused top layer at 15 M rows, 64 -> 128, two graphs,
    rows shuffled: every property of tests/test_fpool_fwd_level_gpu.py on all 428 571 segments (the
    f64 reference walks them in chunks of 1 M rows), the per-segment reference once more on 300
    segments alone, then the backward against identity (iii) in f64, chunk by chunk, on every row.

    Peak device memory about 16 GB: x 3.84 GB, gx 3.84 GB, the CSR view and the winners sorted by
    position 1.6 GB, a dozen [428 571, 128] tables of the reference (f64 / int64) 4.4 GB, f64 chunks
    of 1 M rows (y 0.5 GB, h and its companions 1 GB each).  The forward's reference is freed
    before the backward runs."""
    g = torch.Generator(device=dev).manual_seed(15)
    c = H.build(g, ROWS, SEGS, 64, C, dev, "shuffled", 2)
    name = {1: "f32", 3: "bf16"}[mode]
    fwd3m = dict(zip(H.QUANTITIES, FWD.PARENT_ERR[f"{name}-shuffled-3run-64x128"]))
    o = H.call_forward(c, mode)
    sizes = c.pb.rowptr[1:] - c.pb.rowptr[:-1]
    errs, st, ref = H.check_forward(c, mode, o, f"{name}-15M-2run", parent=fwd3m, factor=4.0,
                                    subset=_spot_segments(sizes, dev))
    del st, ref
    torch.cuda.empty_cache()
    # ---- backward --------------------------------------------------------------------------------
    gout = torch.randn(SEGS, C, device=dev, generator=g)
    c1, c2, c3 = (torch.rand(2, C, device=dev, generator=g) * 0.1 for _ in range(3))
    gr = H.call_backward(c, mode, o, gout, c1, c2, c3)
    berrs, counts = H.backward_errors(c, o, gr, c2, c3)
    print(f"fpool bwd {name}-15M-2run: gx {berrs[0]:.3e} gW {berrs[1]:.3e} sum g' {berrs[2]:.3e} "
          f"sum g'o' {berrs[3]:.3e}")
    assert counts == [p1 - p0 for p0, p1, _ in c.pb.runs]
    assert all(e == e for e in berrs), f"NaN in an output: {berrs}"
    for q, e, b in zip(("gx", "gW", "sum g'", "sum g' o'"), berrs, BWD.PARENT_ERR[(mode, "shuffled")]):
        assert e <= 4 * b, f"{q}: error {e:.3e} against the parent's {b:.3e} at 3 M rows (allowed: x 4)"
