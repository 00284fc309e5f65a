"""The target-order attention backward (`to::attn_bwd_to_kernel<PREC>`, csrc/edge_attn_to.hip) at
level-1 size - 430 000 nodes, up to 6.9 M edges - against the float64 oracle, in the default f32
mode (PREC = 3: split-bf16 products) and the bf16 mode (PREC = 1).

The graphs fix the number of TARGET nodes per 16-edge tile of the target-ordered stream: every node
receives 16, 4 or 1 edges (1, 4 or 16 targets per tile), and one graph makes every node's first
in-edge a self loop.  Checked: the block output, the input gradient (dq, dk, dv through the qkv
Linear), d edge_attr and the weight and bias gradients of the three edge_attr projections.  The f64
reference runs on the GPU."""
import pytest
import torch

from oracle import spt_oracle as O

pytestmark = pytest.mark.gpu

N_NODES, H, D, DIM, F = 430_000, 16, 4, 64, 32


def _graph(gen, n, indeg, loops):
    t = torch.arange(n).repeat_interleave(indeg)
    s = torch.randint(0, n, (t.numel(),), generator=gen)
    if loops:
        s.view(n, indeg)[:, 0] = torch.arange(n)
    p = torch.randperm(t.numel(), generator=gen)
    return torch.stack([s[p], t[p]])


def _err(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    assert a.shape == ref.shape
    return ((a - ref).abs().max() / ref.abs().max().clamp(min=5e-2)).item()


@pytest.mark.parametrize("indeg,loops", [(16, False), (16, True), (4, False), (1, False)],
                         ids=["1-target-per-tile", "1-target-per-tile-loops", "4-targets-per-tile",
                              "16-targets-per-tile"])
@pytest.mark.parametrize("mode,tol", [(2, 2e-5), (3, 2e-2)], ids=["f32", "bf16"])
def test_target_order_backward_at_level1_size_matches_the_f64_oracle(indeg, loops, mode, tol, dev):
    from superpoint_transformer_amd import _lib, nn as N
    gen = torch.Generator().manual_seed(1000 * indeg + loops)
    n = N_NODES
    ei = _graph(gen, n, indeg, loops)
    E = ei.shape[1]
    torch.manual_seed(indeg + 7 * loops)
    blk = N.SelfAttentionBlock(DIM, num_heads=H, out_dim=None, qk_dim=D, in_rpe_dim=F,
                               k_rpe=True, q_rpe=True, v_rpe=True).to(dev)
    x = torch.randn(n, DIM, generator=gen)
    ea = torch.randn(E, F, generator=gen) * 0.5
    gw = torch.randn(n, DIM, generator=gen)
    prev = _lib.lib.spt_attn_use_mfma(mode)
    prev_to = _lib.lib.spt_attn_bwd_el_target_order(1)
    prev_packed = _lib.lib.spt_attn_bwd_packed(2)
    try:
        xd, ead, eid = x.to(dev).requires_grad_(), ea.to(dev).requires_grad_(), ei.to(dev)
        out = blk(xd, eid, edge_attr=ead)
        (out * gw.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        _lib.lib.spt_attn_use_mfma(prev)
        _lib.lib.spt_attn_bwd_el_target_order(prev_to)
        _lib.lib.spt_attn_bwd_packed(prev_packed)

    p = {k: v.detach().double().requires_grad_() for k, v in blk.named_parameters()}
    x64, ea64 = x.to(dev).double().requires_grad_(), ea.to(dev).double().requires_grad_()
    with torch.device(dev):                         # the oracle's own tensors on the GPU as well
        ref = O.self_attention(x64, eid, ea64, p, H, D)
        (ref * gw.to(dev).double()).sum().backward()

    errs = {"out": _err(out, ref), "g_x": _err(xd.grad, x64.grad), "g_edge_attr": _err(ead.grad, ea64.grad)}
    for k, v in blk.named_parameters():
        errs["g_" + k] = _err(v.grad, p[k].grad)
    assert any(k.startswith("g_k_rpe") for k in errs) and any(k.startswith("g_v_rpe") for k in errs)
    bad = {k: e for k, e in errs.items() if not e <= tol}
    assert not bad, f"max err / max|ref| above {tol:g}: {bad}"
    if mode == 3:
        assert errs["g_edge_attr"] > 1e-5           # the bf16 mode really ran: well above f32 round-off
