"""tests/fpool_reference.py (the f64 reference the pool-fused forward's GPU tests compare with)
against the oracle of the same operation - the top layer `oracle.spt_model.mlp` (bias-free Linear
-> GraphNorm -> LeakyReLU) followed by `oracle.spt_oracle.scatter_max` - on the CPU: pooled values
and norm tables to 1e-12 relative, arg rows exactly.  About 5 000 rows in 3 graphs, empty segments,
negative and zero norm weights, shuffled rows; once on all segments and once in small row chunks on
a subset of whole segments (the way the 15 M-row test uses it)."""
import pytest
import torch

import fpool_reference as R
from oracle import spt_model as OM
from oracle import spt_oracle as O

ROWS, SEGS, K, N, B = 5003, 180, 64, 128, 3


def _problem(order):
    from superpoint_transformer_amd import nn as NN
    g = torch.Generator().manual_seed(5)
    live = torch.ones(SEGS, dtype=torch.bool)
    live[[0, 1, 59, 60, 61, 100, 119, 120, SEGS - 1]] = False       # empty: front, run edges, inside, back
    sizes = torch.zeros(SEGS, dtype=torch.long)
    nl = int(live.sum())
    s = torch.randint(1, 50, (nl,), generator=g)
    s[0] += ROWS - int(s.sum())
    assert int(s.min()) >= 1
    sizes[live] = s
    rowptr = torch.zeros(SEGS + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(sizes, 0)
    seg_graph = torch.zeros(SEGS, dtype=torch.long)
    seg_graph[60:120] = 1
    seg_graph[120:] = 2
    runs = [(0, int(rowptr[60]), 0), (int(rowptr[60]), int(rowptr[120]), 1), (int(rowptr[120]), ROWS, 2)]
    si = torch.repeat_interleave(torch.arange(SEGS), sizes)
    if order == "shuffled":
        si = si[torch.randperm(ROWS, generator=g)]
    perm = torch.argsort(si, stable=True)
    x = torch.randn(ROWS, K, generator=g, dtype=R.D) * 2 + 0.5
    # a block of equal rows inside one segment: bitwise equal h, the first one is the arg
    blk = perm[int(rowptr[30]):int(rowptr[31])]
    x[blk[1:]] = 3 * x[blk[1]]
    mlp = NN.MLP([K, N], norm=NN.GraphNorm).double()
    lin, gn, act = mlp.mlp
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g, dtype=R.D) * 0.2)
        gn.weight.copy_(torch.randn(N, generator=g, dtype=R.D))
        pick = torch.randperm(N, generator=g)
        gn.weight[pick[:40]] = -gn.weight[pick[:40]].abs() - 0.05
        gn.weight[pick[40:43]] = 0.0
        gn.bias.copy_(torch.randn(N, generator=g, dtype=R.D) * 0.1)
        gn.mean_scale.copy_(torch.rand(N, generator=g, dtype=R.D))
    pb = R.Problem(
        x=x, perm=perm, rowptr=rowptr, runs=runs, seg_graph=seg_graph, W=lin.weight.detach(),
        pre_am=torch.randn(B, K, generator=g, dtype=R.D) * 0.1,
        pre_scale=torch.rand(B, K, generator=g, dtype=R.D) + 0.5,
        pre_bias=torch.randn(K, generator=g, dtype=R.D) * 0.1, pre_slope=0.2,
        gn_weight=gn.weight.detach(), gn_bias=gn.bias.detach(), gn_mean_scale=gn.mean_scale.detach(),
        eps=gn.eps, slope=act.negative_slope)
    return pb, mlp, si


def _rel(a, r):
    return float((a - r).abs().max() / r.abs().max())


@pytest.mark.parametrize("order", ["shuffled", "csr"])
def test_reference_equals_the_oracle_of_layer_then_pool(order):
    pb, mlp, si = _problem(order)
    batch = pb.seg_graph[si]
    y = (pb.x - pb.pre_am[batch]) * pb.pre_scale[batch] + pb.pre_bias
    y = torch.nn.functional.leaky_relu(y, pb.pre_slope)
    z = OM.mlp(mlp, y, batch, R.D)                                # [rows, N]: the layer's output
    ref, rarg = O.scatter_max(z, si, dim_size=SEGS)
    lin, gn, _ = mlp.mlp
    h = y @ lin.weight.detach().t()

    st = R.statistics(pb, chunk=700)
    for b in range(B):
        hb, yb = h[batch == b], y[batch == b]
        assert _rel(st.gram[b, :K * K].view(K, K), yb.t() @ yb) < 1e-12
        assert _rel(st.gram[b, K * K:K * K + K], yb.sum(0)) < 1e-12
        assert st.gram[b, -1].item() == hb.shape[0] == st.total[b, -1].item()
        assert _rel(st.total[b, :N], hb.sum(0)) < 1e-12
        assert _rel(st.total[b, N:2 * N], (hb * hb).sum(0)) < 1e-12
        # the norm's tables as the oracle's GraphNorm applies them: z = scale (h - am) + bias
        zb = torch.nn.functional.leaky_relu(st.scale[b] * (hb - st.am[b]) + pb.gn_bias, pb.slope)
        assert _rel(zb, z[batch == b]) < 1e-12
        mu = hb.mean(0)
        assert _rel(st.mean[b], mu) < 1e-12
        var = ((hb - pb.gn_mean_scale * mu) ** 2).mean(0)
        assert _rel(st.rstd[b], 1 / torch.sqrt(var + pb.eps)) < 1e-12
    assert abs(st.h_absmax - float(h.abs().max())) <= 1e-12 * st.h_absmax

    def check(segs, po):
        empty = (pb.rowptr[segs + 1] == pb.rowptr[segs])
        assert bool(empty.any()) and bool((~empty).any())
        arg = torch.where(po.argpos < ROWS, pb.perm[po.argpos.clamp(max=ROWS - 1)],
                          torch.full_like(po.argpos, ROWS))
        assert torch.equal(arg, rarg[segs])
        assert _rel(po.out, ref[segs]) < 1e-12
        assert bool((po.out[empty] == 0).all()) and bool((po.raw[empty] == 0).all())
        assert bool((po.argpos[empty] == ROWS).all())
        ne = ~empty
        assert _rel(po.raw[ne], h[arg[ne], torch.arange(N).expand(int(ne.sum()), N)]) < 1e-12
        assert torch.equal(po.h_witness[ne], po.raw[ne])

    all_segs = torch.arange(SEGS)
    full = R.pool_segments(pb, st, all_segs, witness=rarg_positions(pb, rarg))
    check(all_segs, full)
    # the duplicated rows win somewhere, and where they do the arg is the first of them
    blk = pb.perm[int(pb.rowptr[30]):int(pb.rowptr[31])]
    a30 = rarg[30]
    assert int((a30 == blk[1]).sum()) >= 10 and not bool(torch.isin(a30, blk[2:]).any())
    # zero-weight channels: the segment's first row
    zero = pb.gn_weight == 0
    assert int(zero.sum()) == 3
    live = pb.rowptr[1:] > pb.rowptr[:-1]
    assert bool((full.argpos[live][:, zero] == pb.rowptr[:-1][live][:, None]).all())
    # a subset of whole segments, in an arbitrary order, in small blocks
    sub = torch.tensor([SEGS - 1, 30, 0, 7, 60, 119, 121, 59, 150, 2, 100, 99])
    part = R.pool_segments(pb, st, sub, witness=full.argpos[sub], chunk=64)
    check(sub, part)
    assert torch.equal(part.argpos, full.argpos[sub])
    live = ~torch.isinf(part.ext)
    for f in ("raw", "out", "ext"):                 # (a product in other blocks: the last bits may differ)
        assert _rel(getattr(part, f)[live], getattr(full, f)[sub][live]) < 1e-12, f


def rarg_positions(pb, rarg):
    """CSR positions of the oracle's arg rows (n_rows stays n_rows)."""
    inv = torch.empty(ROWS + 1, dtype=torch.long)
    inv[pb.perm] = torch.arange(ROWS)
    inv[ROWS] = ROWS
    return inv[rarg]


def test_bf16_mode_rounds_both_operands_to_nearest_even():
    t = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5, 0.0], dtype=R.D)
    # 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7: ties to even (1); 1 + 3 * 2^-8 ties to 1 + 2^-6
    assert R.round_bf16(t).tolist()[:4] == [1.0, 1.0, 1.015625, -1.0]
    pb, _, _ = _problem("csr")
    pb.bf16 = True
    pos = torch.arange(0, 100)
    y = pb.y_at(pos)
    assert torch.equal(y, y.to(torch.bfloat16).to(R.D))
    assert torch.equal(pb.h_at(pos), y @ pb.W.to(torch.float32).to(torch.bfloat16).to(R.D).t())
