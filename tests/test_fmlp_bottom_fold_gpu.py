"""The chain's bottom layer folded into the backward of the layer above it (DESIGN.md 7.11,
``ops.FOLD_BOTTOM``): where the chain's input needs no gradient, gW0 comes out of the upper layer's
post launch from sums that layer's kernel takes while it holds g' and the tile of x0 - no [rows, 32]
gradient is written or read and the bottom layer has no launch of its own.

Every case runs the two-layer chain's backward twice on the same saved forward - folded, and layer
by layer (the switch off) - and against an f64 restatement of the backward written here, evaluated
at the device's own layer outputs (so that no LeakyReLU kink decides: the masks are the kernel's).

Built pairs: 12 -> 32 under 32 -> 64 (the point MLP: 48-byte rows staged by LDS-DMA, one k block)
and 18 -> 32 under 32 -> 32 (the edge MLP: 72-byte rows, 8-byte aligned, element staging, K0 + 1
padded to two k blocks).  Every case asserts that the folded route really ran: its gW0 comes from
other sums than the layer-by-layer one and is not bitwise equal to it.

Bars.  gW0: the folded route may err at most 4 x what the layer-by-layer route errs against the
f64 reference on the same inputs (three separately rounded terms plus the un-shift), and never more
than the 2e-4-of-max bar tests/test_fused_mlp_gpu.py holds parameter gradients to.  The upper
layer's gW1 and every norm-parameter gradient (they are functions of the statistics p1 / p2 alone)
must be the layer-by-layer route's bit for bit: same operands, same order.

Measured on MI355X (max |error| / max |reference|; folded, layer by layer): see
profiles/r10a_fmlp_bottom_fold.txt."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPE = 0.01
EPS = 1e-5

# K0, N1, rows per run (sorted batch: one graph per run), mean_scale == 1, a column with mean = 10 std
CASES = [
    (12, 64, [16 * 131 + 5], False, False),
    (12, 64, [1029, 11, 1061], False, False),          # 2101 = 16 * 131 + 5 rows, one run under a tile
    (12, 64, [1029, 11, 1061], True, False),
    (12, 64, [16 * 12500 + 5], False, True),           # many workgroups' tables meet; the shift earns its keep
    (12, 64, [16 * 12500 + 5], True, True),
    (18, 32, [16 * 131 + 5], False, False),
    (18, 32, [1029, 11, 1061], False, False),
    (18, 32, [16 * 12500 + 5], False, True),
]


def _inputs(K0, N1, runs, ms_one, offset, dev):
    g = torch.Generator().manual_seed(1000 * K0 + N1 + sum(runs) + 7 * int(ms_one))
    rows = sum(runs)
    x = torch.randn(rows, K0, generator=g)
    x[:, 1] = 0.3 * x[:, 1] - 2.0
    if offset:
        x[:, 3] = x[:, 3] + 10.0                        # mean = 10 x standard deviation
    dims = [K0, 32, N1]
    params = []
    for k, n in zip(dims[:-1], dims[1:]):
        W = torch.randn(n, k, generator=g) / k ** 0.5
        w = 1.0 + 0.3 * torch.randn(n, generator=g)
        w[2] = 0.0                                      # a channel the norm switches off
        w[5] = -0.8                                     # and one it flips
        b = 0.2 * torch.randn(n, generator=g)
        ms = torch.ones(n) if ms_one else 0.5 + 0.7 * torch.rand(n, generator=g)
        params += [W, w, b, ms]
    gy = torch.randn(rows, N1, generator=g)
    batch = torch.cat([torch.full((r,), i, dtype=torch.long) for i, r in enumerate(runs)])
    return x.to(dev), [p.to(dev) for p in params], gy.to(dev), batch.to(dev)


def _graph_norm64(h, batch, B, w, b, ms):
    out = torch.empty_like(h)
    for i in range(B):
        sel = batch == i
        hc = h[sel] - ms * h[sel].mean(0)
        out[sel] = w * hc / torch.sqrt((hc * hc).mean(0) + EPS) + b
    return out


def _reference(x, params, gy, batch, B, hs, tabs):
    """f64 backward of the chain at the device's layer outputs hs, with the kernels' own activation
    masks (sign of fmaf(h - am, scale, bias) in f32 = sign of the same expression in f64)."""
    d = torch.float64
    P = [p.detach().to(d).requires_grad_() for p in params]
    cur = x.to(d)
    for l in range(2):
        W, w, b, ms = P[4 * l: 4 * l + 4]
        z = cur @ W.t()
        h = hs[l].to(d) + (z - z.detach())              # the device's values, the true derivative
        am, sc = tabs[l][2], tabs[l][3]
        bl = batch if B > 1 else torch.zeros_like(batch)
        pre32 = (hs[l] - am[bl]).to(d) * sc[bl].to(d) + params[4 * l + 2].to(d)
        fac = torch.where(pre32 > 0, torch.ones((), dtype=d, device=h.device),
                          torch.full((), SLOPE, dtype=d, device=h.device))
        cur = _graph_norm64(h, batch, B, w, b, ms) * fac
    (cur * gy.to(d)).sum().backward()
    return [p.grad for p in P]


@pytest.mark.parametrize("K0,N1,runs,ms_one,offset", CASES)
def test_folded_bottom_layer_matches_f64_and_the_layer_by_layer_route(K0, N1, runs, ms_one, offset, dev):
    from superpoint_transformer_amd import _lib, ops
    x, params, gy, batch = _inputs(K0, N1, runs, ms_one, offset, dev)
    B, rows = len(runs), sum(runs)
    gr = ops.graph_runs(batch if B > 1 else None, B, rows)
    assert gr is not None and gr.B == B
    built = bool(_lib.lib.spt_fused_linear_bwd_fold_supported(K0, 32, N1, -1))
    assert built, "both shape pairs of this file are built in the default matrix mode"
    _, saved, _, _ = ops._fmlp_forward(x, batch if B > 1 else None, gr, [EPS, EPS], [SLOPE, SLOPE], params)
    meta = (2, gr, [SLOPE, SLOPE], torch.float32, False, -1)

    def backward(fold):
        prev = ops.fold_bottom(fold)
        try:
            gx0, grads = ops._fmlp_backward(saved, meta, gy)
        finally:
            ops.fold_bottom(prev)
        assert gx0 is None
        torch.cuda.synchronize()
        return grads

    new, old = backward(True), backward(False)
    hs = saved[2:4]
    tabs = [tuple(saved[4 + 4 * i: 8 + 4 * i]) for i in range(2)]
    ref = _reference(x, params, gy, batch, B, hs, tabs)

    def err(a, r):
        return ((a.double() - r).abs().max() / r.abs().max().clamp(min=1e-2)).item()

    names = ["gW0", "gn0.weight", "gn0.bias", "gn0.mean_scale", "gW1", "gn1.weight", "gn1.bias", "gn1.mean_scale"]
    e_new = {n: err(a, r) for n, a, r in zip(names, new, ref)}
    e_old = {n: err(a, r) for n, a, r in zip(names, old, ref)}
    tag = f"K0={K0} N1={N1} runs={runs} mean_scale{'=' if ms_one else '!='}1 built={int(built)}"
    for n in names:
        print(f"fold-error {tag} {n}: folded {e_new[n]:.3e} layer-by-layer {e_old[n]:.3e}")
    # the upper layer and the statistics: same operands, same order
    for n, a, o in zip(names[1:], new[1:], old[1:]):
        assert torch.equal(a, o), f"{n}: the folded route moved it"
    for n in names:
        assert e_new[n] <= 2e-4 and e_old[n] <= 2e-4, f"{n}: folded {e_new[n]:.3e} layer-by-layer {e_old[n]:.3e}"
    assert e_new["gW0"] <= 4 * e_old["gW0"], (
        f"gW0: folded {e_new['gW0']:.3e} > 4 x layer-by-layer {e_old['gW0']:.3e}")
    assert not torch.equal(new[0], old[0]), "the folded route was not taken"
