"""Run-to-run reproducibility, bit for bit, of the kernels whose sources say "fixed order:
deterministic" (csrc/graphnorm.hip, fused_mlp.hip, fused_mlp_dma.hip, fused_pool.hip,
skinny_linear.hip, segcsr.hip, usn.hip) and of the attention backward in its source order
(``precision.attention_backward_order("source")``: "no atomics, every gradient bitwise
reproducible run to run").

A tolerance against an f64 oracle cannot see an LDS race, a read of scratch that the kernel never
wrote, or a partial tile read past its rows: each of them moves a value slightly, or only
sometimes.  Here every op runs TWICE on the same inputs and every output and every gradient is
compared by its bit pattern - no tolerance anywhere in this file:

  * run 1 starts with ``ops._WS.clear()``: the scratch buffer of the stream is freshly allocated;
  * between the runs an unrelated op of another family runs on the same stream and the same
    scratch, and one 2048 x 2048 ``torch.matmul``: scratch, LDS and registers hold another
    kernel's leftovers, the allocator's free blocks another op's values;
  * run 2 writes into new output tensors (run 1's are still alive).

No artificial pattern is written into the scratch: a kernel that wrongly read unwritten scratch as
an index would then read far out of range.  Natural leftovers make such a read a mismatch.

Shapes: the smallest that take the kernel and not a torch fallback (4096 rows for the fused MLP and
the skinny Linears, 65 536 edges / rows for the padded attention route and the row-streaming
segment kernels), span several workgroups and end in a partial tile.  Inputs come from the sibling
files' builders.  dW, cross-entropy, the histogram loss, the attention forward and the adjacency
hub have their own such checks (test_skinny_linear_gpu, test_loss_gpu, test_hist_loss_gpu,
test_attention_gpu, test_adjacency_gpu)."""
import copy

import pytest
import torch

import fpool_harness as H
import test_attention_gpu as ATT
import test_fused_mlp_gpu as FM
import test_fused_pool_gpu as FP
import test_prenorm_fused_gpu as PN
import test_segcsr_gpu as SEG
from test_fused_mlp_gpu import gemm_mode  # noqa: F401  (the fixture of the three GEMM modes)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------
# the common procedure
# ---------------------------------------------------------------------------------------------------
def _bits(t):
    """The tensor's bit pattern (NaN payloads and the sign of zero count)."""
    if t.is_floating_point():
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _leftovers_graph_norm(dev):
    from superpoint_transformer_amd import ops
    g = torch.Generator(device=dev).manual_seed(1234)
    x = (torch.randn(20_000, 64, device=dev, generator=g) * 3 - 1).requires_grad_()
    batch = torch.randint(0, 3, (20_000,), device=dev, generator=g)
    w, b, a = (torch.rand(64, device=dev, generator=g).requires_grad_() for _ in range(3))
    ops.graph_norm(x, batch, w, b, a, num_graphs=3, act_slope=0.2).square().sum().backward()


def _leftovers_unit_sphere(dev):
    from superpoint_transformer_amd import ops
    g = torch.Generator(device=dev).manual_seed(4321)
    pos = torch.randn(50_000, 3, device=dev, generator=g) * 7 - 2
    idx = torch.randint(0, 1500, (50_000,), device=dev, generator=g)
    ops.unit_sphere_norm(pos, idx, None, 1500)


def _twice(run, dev, other):
    """``run() -> {name: tensor}`` twice, as the module's docstring lays out; ``other``: the
    unrelated op in between ("graph_norm" or "unit_sphere": of another family than ``run``)."""
    from superpoint_transformer_amd import ops
    torch.cuda.synchronize()
    ops._WS.clear()
    first = run()
    {"graph_norm": _leftovers_graph_norm, "unit_sphere": _leftovers_unit_sphere}[other](dev)
    m = torch.randn(2048, 2048, device=dev)
    m = torch.matmul(m, m)
    del m
    second = run()
    torch.cuda.synchronize()
    assert first.keys() == second.keys() and first
    bad = {}
    for k in first:
        a, b = first[k], second[k]
        assert (a is None) == (b is None), k
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.data_ptr() != b.data_ptr() or a.numel() == 0, f"{k}: run 2 wrote into run 1's tensor"
        n = int((_bits(a) != _bits(b)).sum())
        print(f"  differing elements {k}: {n} of {a.numel()}")
        if n or not torch.equal(_bits(a), _bits(b)):
            bad[k] = n
    assert not bad, f"not bitwise reproducible (differing elements per tensor): {bad}"


def _grads(out, gw, leaves):
    """Backward of sum(out * gw); the gradients of ``leaves`` (a dict) as ``g_<name>``."""
    for t in leaves.values():
        t.grad = None
    (out * gw).sum().backward()
    return {"g_" + k: t.grad for k, t in leaves.items()}


# ---------------------------------------------------------------------------------------------------
# segment sums (csrc/segcsr.hip)
# ---------------------------------------------------------------------------------------------------
_SEG_SHAPES = [c for c in SEG.CASES if c in ((4096 * 3 + 17, 300, 32), (777, 901, 128))]
assert len(_SEG_SHAPES) == 2


@pytest.mark.parametrize("n,nseg,c", _SEG_SHAPES + [(65_536, "lognormal", 128)])
def test_segment_sum_mean_and_gather_backward(n, nseg, c, dev):
    """``segment_reduce`` sum and mean, forward and backward, and ``gather_rows`` backward (a
    segment sum over the gathered rows); at 65 536 x 128 with lognormal segment sizes the
    row-streaming kernels (max + arg included there: the route's own reduction)."""
    from superpoint_transformer_amd import ops
    g = torch.Generator().manual_seed(n + 7 * c)
    if nseg == "lognormal":
        idx, nseg = SEG._segments("lognormal", n, g)
    else:
        idx = torch.randint(0, nseg, (n,), generator=g)
    idx = idx.to(dev)
    x = torch.randn(n, c, generator=g).to(dev)
    src = torch.randn(nseg, c, generator=g).to(dev)
    gw_seg = torch.randn(nseg, c, generator=g).to(dev)
    gw_row = torch.randn(n, c, generator=g).to(dev)
    stream = n >= 65_536

    def run():
        res = {}
        for reduce in ("sum", "mean") + (("max",) if stream else ()):
            xd = x.clone().requires_grad_()
            out = ops.segment_reduce(xd, idx, nseg, reduce)
            res[reduce] = out.detach()
            res.update({f"{reduce}_{k}": v for k, v in _grads(out, gw_seg, {"x": xd}).items()})
        sd = src.clone().requires_grad_()
        rows = ops.gather_rows(sd, idx)
        res["gather"] = rows.detach()
        res.update({f"gather_{k}": v for k, v in _grads(rows, gw_row, {"x": sd}).items()})
        return res

    _twice(run, dev, "graph_norm")


# ---------------------------------------------------------------------------------------------------
# GraphNorm (csrc/graphnorm.hip)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [1.0, 0.01], ids=["plain", "leaky"])
@pytest.mark.parametrize("r,d,B,sorted_batch", [(5000, 32, 3, False), (60_000, 128, 40, False),
                                                (60_000, 128, 40, True)])
def test_graph_norm(r, d, B, sorted_batch, slope, dev):
    """Forward and backward, with and without the fused LeakyReLU; 40 graphs of 128 channels need
    several LDS graph windows.  (The statistics kernels add f64 partials into an LDS table with
    atomics: order-dependent in the last f64 bit, expected to be stable once rounded to f32.)"""
    from superpoint_transformer_amd import ops
    g = torch.Generator().manual_seed(r + d)
    x = (torch.randn(r, d, generator=g) * 2 + 3).to(dev)
    batch = torch.randint(0, B, (r,), generator=g)
    if sorted_batch:
        batch = batch.sort().values
    batch = batch.to(dev)
    w, b = torch.randn(d, generator=g).to(dev), torch.randn(d, generator=g).to(dev)
    a = (1 + 0.3 * torch.randn(d, generator=g)).to(dev)
    gw = torch.randn(r, d, generator=g).to(dev)

    def run():
        leaves = {k: t.clone().requires_grad_() for k, t in (("x", x), ("w", w), ("b", b), ("a", a))}
        y = ops.graph_norm(leaves["x"], batch, leaves["w"], leaves["b"], leaves["a"], eps=1e-5,
                           num_graphs=B, act_slope=slope)
        return {"y": y.detach(), **_grads(y, gw, leaves)}

    _twice(run, dev, "unit_sphere")


# ---------------------------------------------------------------------------------------------------
# fused MLP (csrc/fused_mlp.hip, fused_mlp_dma.hip)
# ---------------------------------------------------------------------------------------------------
def _mlp_case(dims, rows, B, dev, seed):
    from superpoint_transformer_amd import nn as N
    g = torch.Generator().manual_seed(seed)
    mlp = N.MLP(dims, norm=N.GraphNorm)
    with torch.no_grad():
        for p in mlp.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = (torch.randn(rows, dims[0], generator=g) * 2 + 0.5).to(dev)
    batch = (torch.arange(rows) * B // rows).to(dev) if B > 1 else None
    gw = torch.randn(rows, dims[-1], generator=g).to(dev)
    return mlp.to(dev), x, batch, gw


def _run_mlp(mlp, x, batch, B, gw):
    m = copy.deepcopy(mlp)
    xd = x.clone().requires_grad_()
    y = m(xd, batch=batch, batch_size=B)
    assert type(y.grad_fn).__name__.startswith("_FusedMLP"), "the fused route did not run"
    (y * gw).sum().backward()
    return {"y": y.detach(), "g_x": xd.grad, **{"g_" + k: p.grad for k, p in m.named_parameters()}}


@pytest.mark.parametrize("dims,rows,B", [([12, 32, 64, 128], 40_001, 3), ([132, 64, 64], 30_000, 1)])
def test_fused_mlp(dims, rows, B, gemm_mode, dev):
    """``nn.MLP`` on the fused route, forward and backward, in the three GEMM modes."""
    mlp, x, batch, gw = _mlp_case(dims, rows, B, dev, rows + B)
    _twice(lambda: _run_mlp(mlp, x, batch, B, gw), dev, "unit_sphere")


@pytest.mark.parametrize("precision_mode", ["f32", "bf16"])
@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "dense"])
@pytest.mark.parametrize("K,N", [(64, 128), (32, 64)])
def test_lds_dma_backward(K, N, pooled, precision_mode, dev):
    """The LDS-DMA staged backward (``spt_fused_linear_bwd_use_dma(1)``) of a K -> N top layer at
    10 007 rows (a short last tile): dense, and with the max-pool's backward inside (the
    materialised MLP -> pool route, the pool-fused top layer switched off)."""
    from superpoint_transformer_amd import _lib, ops, precision
    dims = {(64, 128): [12, 32, 64, 128], (32, 64): [12, 32, 64]}[(K, N)]
    rows, nseg = 10_007, 300
    gen = torch.Generator().manual_seed(rows + K + N)
    mlp, x, _, _, si, gout = FP._problem(gen, rows, nseg, 1, dims, dev)
    mlp, x, si, gout = mlp.to(dev), x.to(dev), si.to(dev), gout.to(dev)
    gw = torch.randn(rows, N, generator=gen).to(dev)

    def run():
        if not pooled:
            return _run_mlp(mlp, x, None, 1, gw)
        m = copy.deepcopy(mlp)
        xd = x.clone().requires_grad_()
        out = m.forward_max_pooled(xd, si, nseg, batch=None, batch_size=1)
        assert out is not None and not getattr(out.grad_fn, "pool_fused", False)
        (out * gout).sum().backward()
        return {"out": out.detach(), "g_x": xd.grad, **{"g_" + k: p.grad for k, p in m.named_parameters()}}

    prev_dma = _lib.lib.spt_fused_linear_bwd_use_dma(1)
    prev_pool = ops.pool_in_forward(False)
    try:
        with precision.matrix_precision(precision_mode):
            _twice(run, dev, "unit_sphere")
    finally:
        ops.pool_in_forward(prev_pool)
        _lib.lib.spt_fused_linear_bwd_use_dma(prev_dma)


# ---------------------------------------------------------------------------------------------------
# pool-fused top layer (csrc/fused_pool.hip) through the C entries
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3, 3 | H.X_BF16], ids=["f32", "bf16", "bf16-rows"])
@pytest.mark.parametrize("order,graphs", [("csr", 1), ("shuffled", 1), ("shuffled", 3)])
def test_pool_fused_top_layer(order, graphs, mode, dev):
    """Forward (out, arg, raw, Gram record, tables) and backward (gm, gx, gW, the previous norm's
    sums) of the 64 -> 128 unit on the harness' smallest problem (40 000 rows, 1000 segments: empty
    segments, equal rows, negative and zero norm weights, run boundaries off the 16-row grid), rows
    in CSR order and shuffled, one graph and three; default mode, bf16 operands, bf16 rows."""
    from superpoint_transformer_amd import _lib
    K, N = 64, 128
    g = torch.Generator(device=dev).manual_seed(3)
    c = H.build(g, 40_000, 1000, K, N, dev, order, graphs, in16=bool(mode & H.X_BF16))
    assert _lib.lib.spt_fused_linear_pool_supported(K, N, mode)
    B = c.pb.num_graphs
    gout = torch.randn(c.num_seg, N, device=dev, generator=g)
    c1, c2, c3 = (torch.rand(B, N, device=dev, generator=g) * 0.1 for _ in range(3))

    def run():
        o = H.call_forward(c, mode)
        _lib.check(o.status, "spt_fused_linear_fwd_pool_runs_f32")
        gr = H.call_backward(c, mode, o, gout, c1, c2, c3)
        _lib.check(gr.status, "spt_fused_linear_bwd_pool_runs_f32")
        res = {f: getattr(o, f) for f in ("out", "arg", "argpos", "raw", "gram", "total", "mean", "rstd",
                                           "am", "scale")}
        res.update({f: getattr(gr, f) for f in ("gm", "gx", "gW", "ptot")})
        return res

    _twice(run, dev, "graph_norm")


# ---------------------------------------------------------------------------------------------------
# skinny Linears (csrc/skinny_linear.hip): the entries without a reproducibility check of their own
# ---------------------------------------------------------------------------------------------------
_SKINNY = [(e, K, N) for K, N in ((64, 192), (132, 128)) for e in ("forward", "input-grad")]
# (the residual epilogue and the folded pre-norm are built for K in {32, 64, 128} only)
_SKINNY += [("linear-residual", 64, 192), ("norm-linear", 64, 192)]


@pytest.mark.parametrize("mode", [0, 1], ids=["f32-pipe", "split-bf16"])
@pytest.mark.parametrize("rows", [4099, 70_001])
@pytest.mark.parametrize("entry,K,N", _SKINNY)
def test_skinny_linear_entries(entry, K, N, rows, mode, dev):
    """``_skinny_launch`` (forward), ``spt_skinny_linear_wt_m_f32`` (dX, the weight read
    transposed), ``ops.linear_residual`` and ``ops.norm_linear`` (forward and every gradient)."""
    from superpoint_transformer_amd import _lib, ops, precision
    g = torch.Generator().manual_seed(rows + K + N)
    x = (torch.randn(rows, K, generator=g) * 2 + 0.5).to(dev)
    W = (torch.randn(N, K, generator=g) * 0.2).to(dev)
    b = (torch.randn(N, generator=g) * 0.1).to(dev)
    gy = torch.randn(rows, N, generator=g).to(dev)
    res = torch.randn(rows, N, generator=g).to(dev)
    B = 3
    batch = (torch.arange(rows) * B // rows).to(dev)
    gn = [(torch.rand(K, generator=g) + 0.5).to(dev) for _ in range(3)]
    gres = torch.randn(rows, K, generator=g).to(dev)
    assert precision._MODES[{0: "f32-exact", 1: "f32"}[mode]][2] == mode

    def run():
        if entry == "forward":
            assert ops._skinny_ok(x, W)
            return {"y": ops._skinny_launch(x, W, b, mode)}
        if entry == "input-grad":
            assert _lib.lib.spt_skinny_linear_supported(N, K) and K % 4 == 0 and K >= 64
            return {"g_x": ops._input_grad(gy, W, mode)}
        leaves = {k: t.clone().requires_grad_() for k, t in (("x", x), ("W", W), ("b", b))}
        with precision.matrix_precision({0: "f32-exact", 1: "f32"}[mode]):
            if entry == "linear-residual":
                leaves["res"] = res.clone().requires_grad_()
                assert ops.linear_residual_ok(leaves["res"], W)
                y = ops.linear_residual(leaves["x"], leaves["W"], leaves["b"], leaves["res"])
                assert type(y.grad_fn).__name__.startswith("_ResidualLinear")
                return {"y": y.detach(), **_grads(y, gy, leaves)}
            leaves.update({k: t.clone().requires_grad_() for k, t in zip(("gn_w", "gn_b", "gn_a"), gn)})
            assert ops.norm_linear_ok(x, batch, B, W)
            y, xres = ops.norm_linear(leaves["x"], batch, B, leaves["gn_w"], leaves["gn_b"], leaves["gn_a"],
                                      1e-5, leaves["W"], leaves["b"])
            for t in leaves.values():
                t.grad = None
            ((y * gy).sum() + (xres * gres).sum()).backward()
            return {"y": y.detach(), **{"g_" + k: t.grad for k, t in leaves.items()}}

    _twice(run, dev, "unit_sphere" if entry == "norm-linear" else "graph_norm")


# ---------------------------------------------------------------------------------------------------
# attention in the source order (csrc/edge_attn*.hip)
# ---------------------------------------------------------------------------------------------------
def _attention_case(n, deg, H_, D, Dv, F, dev, blocks=1):
    from superpoint_transformer_amd import nn as N
    gen = torch.Generator().manual_seed(n * 7 + H_ + F + Dv)
    dim = H_ * Dv
    ei = ATT._rand_graph(gen, n, deg)
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)].to(dev)        # unsorted sources
    blks = [N.SelfAttentionBlock(dim, num_heads=H_, out_dim=None, qk_dim=D, in_rpe_dim=F,
                                 k_rpe=True, q_rpe=True, v_rpe=True).to(dev) for _ in range(blocks)]
    x = torch.randn(n, dim, generator=gen).to(dev)
    ea = (torch.randn(ei.shape[1], F, generator=gen) * 0.5).to(dev)
    gw = torch.randn(n, dim, generator=gen).to(dev)
    return blks, ei, x, ea, gw


@pytest.mark.parametrize("n,deg,H_,D,Dv,F", [
    (5000, 16.0, 16, 4, 4, 32),        # > 65 536 edges: the matrix-pipe route, edge-lane backward
    (700, 3.0, 16, 4, 4, 32),          # few edges, fewer rows than the skinny Linears take
    (5000, 16.0, 16, 4, 8, 32),        # SPT-128: 16 heads of value dim 8, split onto two passes
    (5000, 16.0, 16, 2, 1, 16),        # nano: zero-padded onto the matrix-pipe shape
    # fewer than 1024 tiles of 16 edges: one tile per wave pair, and at ~25 edges per node most
    # nodes span three tiles, i.e. three pairs (the shape of a train step's upper levels: dq of
    # such a node used to be three float atomics in the order the pairs ran)
    (600, 24.0, 16, 4, 4, 32),
], ids=["spt64-5000", "spt64-700", "spt128-split", "nano-padded", "spt64-600-one-tile-per-pair"])
def test_attention_block_in_source_order(n, deg, H_, D, Dv, F, dev):
    """``nn.SelfAttentionBlock`` under ``attention_backward_order("source")``: the output and the
    gradients of x, edge_attr and every parameter (the three RPE weights among them)."""
    from superpoint_transformer_amd import precision
    (blk,), ei, x, ea, gw = _attention_case(n, deg, H_, D, Dv, F, dev)

    def run():
        xd, ead = x.clone().requires_grad_(), ea.clone().requires_grad_()
        blk.zero_grad(set_to_none=True)
        out = blk(xd, ei, edge_attr=ead)
        (out * gw).sum().backward()
        return {"out": out.detach(), "g_x": xd.grad, "g_edge_attr": ead.grad,
                **{"g_" + k: p.grad for k, p in blk.named_parameters()}}

    with precision.attention_backward_order("source"):
        _twice(run, dev, "graph_norm")


def test_shared_edge_attr_gradient_in_source_order(dev):
    """Three chained blocks of a stage accumulating d edge_attr in one buffer
    (``ops.EdgeAttrGradShare``), in the source order."""
    from superpoint_transformer_amd import ops, precision
    blocks, ei, x, ea, gw = _attention_case(5000, 16.0, 16, 4, 4, 32, dev, blocks=3)

    def run():
        xd, ead = x.clone().requires_grad_(), ea.clone().requires_grad_()
        share = ops.EdgeAttrGradShare()
        h = xd
        for b in blocks:
            b.zero_grad(set_to_none=True)
            h = h + b(h, ei, edge_attr=ead, ea_grad=share)
        (h * gw).sum().backward()
        res = {"out": h.detach(), "g_x": xd.grad, "g_edge_attr": ead.grad}
        for i, b in enumerate(blocks):
            res.update({f"g_{i}.{k}": p.grad for k, p in b.named_parameters()})
        return res

    with precision.attention_backward_order("source"):
        _twice(run, dev, "graph_norm")


# ---------------------------------------------------------------------------------------------------
# UnitSphereNorm (csrc/usn.hip), edge-affinity features
# ---------------------------------------------------------------------------------------------------
def test_unit_sphere_norm_and_assemble(dev):
    from superpoint_transformer_amd import ops
    n, nseg, cx = 100_003, 2900, 128
    g = torch.Generator().manual_seed(n + cx)
    pos = (torch.randn(n, 3, generator=g) * 5 + 20).to(dev)
    idx = torch.randint(0, nseg, (n,), generator=g).to(dev)
    w = torch.randint(0, 300, (n,), generator=g).to(dev)
    x = torch.randn(n, cx, generator=g).to(dev)
    gw = torch.randn(n, cx + 4, generator=g).to(dev)

    def run():
        npos, diam = ops.unit_sphere_norm(pos, idx, w, nseg)
        xa = x.clone().requires_grad_()
        out, diam2 = ops.unit_sphere_assemble(xa, pos, idx, w, nseg)
        (out * gw).sum().backward()
        return {"pos": npos, "diameter": diam, "assembled": out.detach(), "assembled_diameter": diam2,
                "g_x": xa.grad}

    _twice(run, dev, "graph_norm")


def test_edge_affinity_features(dev):
    from superpoint_transformer_amd import ops
    g = torch.Generator().manual_seed(2)
    n, c, e = 700, 64, 5000
    x = torch.randn(n, c, generator=g)
    x[5] = x[9]                                          # an exact tie: sign(0) = 0 in the backward
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[:, 0] = torch.tensor([5, 9])
    x, ei = x.to(dev), ei.to(dev)
    gw = torch.randn(e, 2 * c, generator=g).to(dev)

    def run():
        xd = x.clone().requires_grad_()
        out = ops.edge_affinity_features(xd, ei)
        (out * gw).sum().backward()
        return {"out": out.detach(), "g_x": xd.grad}

    _twice(run, dev, "graph_norm")
