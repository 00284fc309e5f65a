"""The sparse convolution on the device (csrc/sparse_conv.hip) against the float64
dense twin of tests/sparse_conv_reference.py: the kernel map, the forward and the three gradients.

Bounds used below, and where they come from:
  * integer operands in [-8, 8]: every product and every partial sum is an integer below 2^24
    (at most 343 * 64 * 64 = 1.4e6 per output, N * 64 per dW entry with N <= 1003), so f32 is
    exact and the device must EQUAL the twin;
  * random f32 operands: at most 4 x the error torch's own f32 CPU ``conv3d`` makes on the same
    dense inputs against the twin, per case and per output, measured in the same test (the table
    is printed; profiles/r23a_sparse_conv_errors.txt is one run of it);
  * device against the f32 CPU composition on 50 000 voxels: both sum the same products in f32 in
    different orders, so each is within n * eps * sum|terms| of the exact value (n = the number
    of summands): the bound is twice that, with sum|terms| from the composition on absolute values
    in f64;
  * networks (SparseCNN, PointStage, SPT): three f32 layers of at most 27 * 32 = 864 summands
    each (relative error at most 864 * 2^-24 = 5e-5 per layer in the worst case) through norms
    whose division by the standard deviation is well conditioned on random features: 1e-3 of the
    largest reference magnitude, per tensor.

PointStage and SPT are compared with THE SAME modules on the torch composition of the CPU route
(``sparse.composition_only()``), run on device tensors: GraphNorm and the MLP kernels of those
modules exist on the device only, so the modules as a whole cannot run on CPU tensors."""
import numpy as np
import pytest
import torch

import sparse_conv_reference as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAMES = ("out", "dX", "dW", "dbias")


def _operands(n, ci, co, K, seed, integer):
    g = torch.Generator().manual_seed(seed)
    shape = (K ** 3, ci, co) if K > 1 else (ci, co)
    if integer:
        def draw(*s):
            return torch.randint(-8, 9, s, generator=g).float()
    else:
        def draw(*s):
            return torch.randn(*s, generator=g)
    return draw(n, ci), draw(*shape), draw(co), draw(n, co)


def _device(S, dev, coords, batch, K, d, x, W, b, gout, kmap=None):
    if kmap is None:
        kmap = S.build_kernel_map(coords.to(dev), None if batch is None else batch.to(dev), K, d)
    xs, Ws = x.to(dev).requires_grad_(), W.to(dev).requires_grad_()
    bs = None if b is None else b.to(dev).requires_grad_()
    out = S.sparse_conv3d(xs, Ws, kmap, bs)
    out.backward(gout.to(dev))
    res = (out.detach(), xs.grad, Ws.grad, None if bs is None else bs.grad)
    return kmap, tuple(None if t is None else t.cpu() for t in res)


def _cloud(n, seed, batches=2):
    extent = 3
    while batches * extent ** 3 < 3 * n:
        extent += 1
    return R.random_cloud(n, extent, seed, batches if n >= batches else 1)


CASES = ([(n, 3, 32, 3, 1) for n in (1, 15, 17, 63, 65, 1003)]
         + [(65, ci, co, 3, 1) for ci in (1, 3, 7, 32) for co in (16, 32, 64)]
         + [(65, 7, 16, K, d) for K in (1, 3, 7) for d in (1, 2)])


@pytest.mark.parametrize("n,ci,co,K,d", CASES)
def test_map_forward_and_gradients(n, ci, co, K, d, dev):
    from superpoint_transformer_amd import sparse as S
    assert S.kernel_supported(ci, co)
    coords, batch = _cloud(n, seed=n + ci + co + K + d)
    # the map
    kmap = S.build_kernel_map(coords.to(dev), None if batch is None else batch.to(dev), K, d)
    assert R.map_triples(kmap) == sorted(R.pairs_dense(coords, batch, K, d))
    assert kmap.rowptr.cpu().tolist()[-1] == kmap.num_pairs
    # integer operands: equality with the twin
    x, W, b, gout = _operands(n, ci, co, K, 1, integer=True)
    _, got = _device(S, dev, coords, batch, K, d, x, W, b, gout, kmap)
    want = R.conv_with_grads(x, W, coords, batch, K, d, b, gout)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and torch.equal(g.double(), w), f"{name}: integer case differs"
    # twice the same bits
    _, again = _device(S, dev, coords, batch, K, d, x, W, b, gout, kmap)
    for name, g, a in zip(NAMES, got, again):
        assert torch.equal(g.view(torch.int32), a.view(torch.int32)), f"{name}: two runs differ"
    # random f32 operands: within 4 x torch's own f32 error
    x, W, b, gout = _operands(n, ci, co, K, 2, integer=False)
    _, got = _device(S, dev, coords, batch, K, d, x, W, b, gout, kmap)
    want = R.conv_with_grads(x, W, coords, batch, K, d, b, gout)
    f32 = R.conv_with_grads(x, W, coords, batch, K, d, b, gout, dtype=torch.float32)
    lines, bad = [], []
    for name, g, w, f in zip(NAMES, got, want, f32):
        err = (g.double() - w).abs().max().item()
        ref = (f.double() - w).abs().max().item()
        lines.append(f"n={n} ci={ci} co={co} K={K} d={d} {name}: device {err:.3e} torch-f32 {ref:.3e}")
        if err > 4 * ref:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "; ".join(bad)
    _, again = _device(S, dev, coords, batch, K, d, x, W, b, gout, kmap)
    for name, g, a in zip(NAMES, got, again):
        assert torch.equal(g.view(torch.int32), a.view(torch.int32)), f"{name}: two runs differ"


def test_full_block_has_all_343_neighbours(dev):
    from superpoint_transformer_amd import sparse as S
    coords = R.full_block(9)
    x, W, b, gout = _operands(729, 3, 16, 7, 3, integer=True)
    kmap, got = _device(S, dev, coords, None, 7, 1, x, W, b, gout)
    counts = (kmap.rowptr[1:] - kmap.rowptr[:-1]).cpu()
    inner = ((coords >= 3) & (coords <= 5)).all(1)
    assert int(inner.sum()) == 27 and bool((counts[inner] == 343).all())
    assert int(counts.max()) == 343 and int(counts.min()) == 64          # a corner: 4^3
    for i in inner.nonzero().flatten().tolist():
        assert kmap.off[kmap.rowptr[i]:kmap.rowptr[i + 1]].cpu().tolist() == list(range(343))
    want = R.conv_with_grads(x, W, coords, None, 7, 1, b, gout)
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g.double(), w), name


@pytest.mark.parametrize("K,d", [(1, 1), (3, 1), (7, 2)])
def test_lone_voxel_has_only_the_centre(K, d, dev):
    from superpoint_transformer_amd import sparse as S
    coords = torch.tensor([[5, -2, 7]])
    x, W, b, gout = _operands(1, 3, 16, K, 4, integer=True)
    kmap, got = _device(S, dev, coords, None, K, d, x, W, b, gout)
    assert kmap.num_pairs == 1 and kmap.off.cpu().tolist() == [K ** 3 // 2]
    assert kmap.nbr.cpu().tolist() == [0] and kmap.rowptr.cpu().tolist() == [0, 1]
    Wc = W.reshape(K ** 3, 3, 16)[K ** 3 // 2]
    assert torch.equal(got[0], x @ Wc + b)
    assert torch.equal(got[1], gout @ Wc.t()) and torch.equal(got[3], gout[0])
    dW = torch.zeros(K ** 3, 3, 16)
    dW[K ** 3 // 2] = x.t() @ gout
    assert torch.equal(got[2].reshape(K ** 3, 3, 16), dW)


def test_plane_and_shell_against_the_cpu_route(dev):
    from superpoint_transformer_amd import sparse as S
    coords, batch = R.plane_and_shell()
    n = coords.shape[0]
    assert 40000 < n < 60000
    ci, co, K = 7, 32, 3
    x, W, b, gout = _operands(n, ci, co, K, 5, integer=False)
    kmap, got = _device(S, dev, coords, batch, K, 1, x, W, b, gout)
    cmap = S.build_kernel_map(coords, batch, K, 1)
    for name in ("rowptr", "nbr", "off", "row"):
        assert torch.equal(getattr(kmap, name).cpu(), getattr(cmap, name)), name
    perm, optr = kmap.by_offset()
    tperm, toptr = cmap.by_offset_torch()
    assert torch.equal(perm.cpu().long(), tperm) and torch.equal(optr.cpu().long(), toptr)

    def route(x, W, b, gout, dtype):
        xs, Ws, bs = (t.detach().clone().to(dtype).requires_grad_() for t in (x, W, b))
        out = S.sparse_conv3d(xs, Ws, cmap, bs)
        out.backward(gout.to(dtype))
        return out.detach(), xs.grad, Ws.grad, bs.grad

    cpu = route(x, W, b, gout, torch.float32)
    mag = route(x.abs(), W.abs(), b.abs(), gout.abs(), torch.float64)
    terms = (27 * ci + 1, 27 * co, int((toptr[1:] - toptr[:-1]).max()), n)
    for name, g, c, m, t in zip(NAMES, got, cpu, mag, terms):
        over = ((g.double() - c.double()).abs() - 2 * t * EPS * m).max().item()
        print(f"{name}: max |device - cpu| {(g - c).abs().max().item():.3e}, bound margin {-over:.3e}")
        assert over <= 0, f"{name}: device and CPU route differ beyond the summation bound"


def test_shuffled_order_gives_the_same_rows(dev):
    from superpoint_transformer_amd import sparse as S
    coords, batch = R.random_cloud(700, 9, 11, batches=2)
    key = ((batch * 64 + coords[:, 2]) * 64 + coords[:, 1]) * 64 + coords[:, 0]
    order = torch.argsort(key)
    x, W, b, gout = _operands(700, 7, 32, 3, 6, integer=False)
    _, a = _device(S, dev, coords, batch, 3, 1, x, W, b, gout)
    _, s = _device(S, dev, coords[order], batch[order], 3, 1, x[order], W, b, gout[order])
    for k in (0, 1):
        assert torch.equal(a[k][order].view(torch.int32), s[k].view(torch.int32)), NAMES[k]


def test_negative_coordinates_and_identical_items(dev):
    from superpoint_transformer_amd import sparse as S
    coords, _ = R.random_cloud(300, 8, 12)
    x, W, b, gout = _operands(300, 3, 16, 3, 7, integer=False)
    m0, a = _device(S, dev, coords, None, 3, 1, x, W, b, gout)
    m1, s = _device(S, dev, coords - 1000, None, 3, 1, x, W, b, gout)
    m2, f = _device(S, dev, (coords - 1000).float(), None, 3, 1, x, W, b, gout)
    for m in (m1, m2):
        assert R.map_triples(m) == R.map_triples(m0)
    for u, v, w in zip(a, s, f):
        assert torch.equal(u, v) and torch.equal(u, w)
    # two items with the same coordinates and other features: neighbours never cross
    x2 = _operands(300, 3, 16, 3, 8, integer=False)[0]
    both = torch.cat([coords, coords])
    batch = torch.cat([torch.zeros(300, dtype=torch.long), torch.ones(300, dtype=torch.long)])
    mb, t = _device(S, dev, both, batch, 3, 1, torch.cat([x, x2]), W, b, torch.cat([gout, gout]))
    assert mb.num_pairs == 2 * m0.num_pairs
    assert torch.equal(batch[mb.row.cpu().long()], batch[mb.nbr.cpu().long()])
    _, a2 = _device(S, dev, coords, None, 3, 1, x2, W, b, gout)
    assert torch.equal(t[0][:300], a[0]) and torch.equal(t[0][300:], a2[0])
    assert torch.equal(t[1][:300], a[1]) and torch.equal(t[1][300:], a2[1])


@pytest.mark.parametrize("K,d", [(3, 1), (3, 2), (7, 1)])
@pytest.mark.parametrize("pow2", [False, True])
def test_aliasing_traps(K, d, pow2, dev):
    from superpoint_transformer_amd import sparse as S
    for coords, batch, (i, j) in R.aliasing_traps(K, d, pow2):
        kmap = S.build_kernel_map(coords.to(dev), batch.to(dev), K, d)
        triples = R.map_triples(kmap)
        pairs = {(a, c) for a, _, c in triples}
        assert (i, j) not in pairs and (j, i) not in pairs
        assert triples == sorted(R.pairs_dense(coords, batch, K, d))


def test_map_with_a_key_wider_than_32_bits(dev):
    """Three 3 x 3 x 3 blocks far apart in two batch items: 14 + 14 + 13 + 1 key bits, so the keys
    are sorted as two words (csrc/sorted_runs.hpp).  The device map must be the CPU route's, pair
    for pair - also on a workspace of exactly the promised size between guards, NaN-filled."""
    from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors
    from superpoint_transformer_amd import sparse as S
    offsets = torch.tensor([[0, 0, 0], [5000, 5000, 5000], [-5000, 9000, 2000]])
    coords = torch.cat([R.full_block(3) + o for o in offsets])
    batch = torch.tensor([0, 1, 1]).repeat_interleave(27)
    order = torch.randperm(81, generator=torch.Generator().manual_seed(81))
    coords, batch = coords[order], batch[order]
    cols = [coords[:, 0], coords[:, 1], coords[:, 2], batch]
    _, bits, total = S._key_layout([int(v.min()) for v in cols], [int(v.max()) for v in cols], 1)
    assert total > 32 and max(bits) <= 32, (bits, total)
    cmap = S.build_kernel_map(coords, batch, 3, 1)
    assert cmap.num_pairs == 3 * 7 ** 3             # 7 pairs within reach per axis, no block meets another
    arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        guarded = S.build_kernel_map(coords.to(dev), batch.to(dev), 3, 1)
    assert len(arena.sizes()) >= 1
    for kmap in (S.build_kernel_map(coords.to(dev), batch.to(dev), 3, 1), guarded):
        assert kmap.num_pairs == cmap.num_pairs
        for name in ("rowptr", "nbr", "off", "row"):
            assert torch.equal(getattr(kmap, name).cpu(), getattr(cmap, name)), name


def test_quantize_point_coordinates_on_the_device(dev):
    from superpoint_transformer_amd import sparse as S
    from superpoint_transformer_amd.data import NAG, Data
    from superpoint_transformer_amd.transforms import QuantizePointCoordinates
    g = torch.Generator().manual_seed(4)
    n = 500
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 2.0
    batch = (torch.arange(n) >= 300).long()
    sup = torch.arange(n) % 7

    def nag():
        d0 = Data(pos=pos.to(dev), x=torch.arange(n, dtype=torch.float32).view(-1, 1).to(dev),
                  super_index=sup.to(dev), batch=batch.to(dev))
        return NAG([d0, Data(pos=torch.zeros(7, 3, device=dev))])

    out = {neg: QuantizePointCoordinates(0.2, allow_negative_coords=neg)(nag()) for neg in (False, True)}
    c = torch.round(pos / 0.2).long()
    c0 = c - c.min(0).values
    ext = c0.max(0).values + 1
    key = ((batch * ext[2] + c0[:, 2]) * ext[1] + c0[:, 1]) * ext[0] + c0[:, 0]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    last = torch.zeros(uniq.numel(), dtype=torch.long)
    last.scatter_reduce_(0, inv, torch.arange(n), "amax", include_self=False)
    want = torch.round(pos / 0.2)[last]
    assert torch.equal(out[True][0].coords.cpu(), want)
    assert torch.equal(out[False][0].coords.cpu(), want - want.min(0, keepdim=True).values)
    assert float(out[True][0].coords.min()) < 0 and float(out[False][0].coords.min()) == 0
    for o in out.values():
        assert torch.equal(o[0].x.cpu().flatten().long(), last)
    maps = [S.build_kernel_map(o[0].coords, o[0].batch, 3, 1) for o in out.values()]
    assert R.map_triples(maps[0]) == R.map_triples(maps[1])
    assert R.map_triples(maps[0]) == sorted(R.pairs_dense(want.long(), batch[last], 3, 1))


def _graph_norm64(x, batch, weight, bias, mean_scale, eps=1e-5):
    nb = int(batch.max()) + 1
    cnt = torch.bincount(batch, minlength=nb).double().view(-1, 1)
    mean = torch.zeros(nb, x.shape[1], dtype=x.dtype).index_add(0, batch, x) / cnt
    out = x - mean[batch] * mean_scale
    var = torch.zeros(nb, x.shape[1], dtype=x.dtype).index_add(0, batch, out * out) / cnt
    return weight * out / (var[batch] + eps).sqrt() + bias


def test_sparse_cnn_against_the_twin(dev):
    from superpoint_transformer_amd.nn.sparse import SparseCNN, SparseTensor
    coords, batch = R.random_cloud(300, 8, 21, batches=2)
    order = torch.argsort(batch, stable=True)               # GraphNorm's graphs are contiguous
    coords, batch = coords[order], batch[order]
    cnn = SparseCNN([5, 32, 32, 32], [7, 3, 3], 1, activation=torch.nn.LeakyReLU(0.01)).to(dev)
    with torch.no_grad():
        for blk in cnn:                                     # (away from the identity norm)
            blk.norm.weight.uniform_(0.5, 1.5)
            blk.norm.bias.uniform_(-0.5, 0.5)
            blk.norm.mean_scale.uniform_(0.5, 1.5)
    x = torch.randn(300, 5)
    gout = torch.randn(300, 32)
    xs = x.to(dev).requires_grad_()
    st = SparseTensor(coords=torch.cat([batch.view(-1, 1), coords], 1).int().to(dev), feats=xs)
    out = cnn(st, batch=batch.to(dev)).F
    out.backward(gout.to(dev))
    assert len(st._maps) == 2                               # (7, 1) and (3, 1): shared by blocks 2, 3
    params = {k: v.detach().cpu().double().requires_grad_() for k, v in cnn.named_parameters()}
    x64 = x.double().requires_grad_()
    h = x64
    for i, K in enumerate((7, 3, 3)):
        h = R.conv_dense(h, params[f"{i}.conv.kernel"], coords, batch, K, 1)
        h = _graph_norm64(h, batch, params[f"{i}.norm.weight"], params[f"{i}.norm.bias"],
                          params[f"{i}.norm.mean_scale"])
        h = torch.nn.functional.leaky_relu(h, 0.01)
    h.backward(gout.double())
    pairs = [("out", out.detach().cpu(), h.detach()), ("dX", xs.grad.cpu(), x64.grad)]
    pairs += [(k, p.grad.cpu(), params[k].grad) for k, p in cnn.named_parameters()]
    for name, g, w in pairs:
        err = (g.double() - w).abs().max().item()
        print(f"{name}: {err:.3e} of {w.abs().max().item():.3e}")
        assert err <= 1e-3 * w.abs().max().item(), name


def _grads(module):
    return {k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}


def _close(name, a, b):
    err = (a.double() - b.double()).abs().max().item()
    assert err <= 1e-3 * max(b.abs().max().item(), 1e-30), f"{name}: {err:.3e}"


@pytest.mark.parametrize("on_cnn", [True, False])
def test_point_stage_with_cnn_blocks(on_cnn, dev):
    from superpoint_transformer_amd import sparse as S
    from superpoint_transformer_amd.nn import GraphNorm, PointStage
    n, nsup = 600, 20
    coords, batch = R.random_cloud(n, 10, 31, batches=2)
    order = torch.argsort(batch, stable=True)
    coords, batch = coords[order].to(dev), batch[order].to(dev)
    inj = 3 + 1
    in_mlp = [16 + 4 + inj, 32, 32] if on_cnn else [4 + inj, 32, 32]
    stage = PointStage(in_mlp, use_pos=True, use_diameter_parent=True, cnn_blocks=True,
                       cnn=[6, 16, 16], cnn_kernel_size=3, cnn_dilation=1, cnn_norm=GraphNorm,
                       cnn_activation=torch.nn.LeakyReLU(), point_mlp_on_cnn_feats=on_cnn).to(dev)
    x = torch.randn(n, 6, device=dev)
    x_mlp = torch.randn(n, 4, device=dev)
    pos = torch.randn(n, 3, device=dev)
    sup = (torch.arange(n, device=dev) * nsup) // n
    gout = None
    res = {}
    for route in ("kernel", "composition"):
        stage.zero_grad()
        xs = x.clone().requires_grad_()
        with S.composition_only(route == "composition"):
            out, diam = stage(xs, batch, pos=pos, super_index=sup, coords=coords, batch=batch,
                              x_mlp=x_mlp, num_super=nsup, num_graphs=2)
            assert out.shape == (n, 32 if on_cnn else 16 + 32) and diam.shape[0] == nsup
            if gout is None:
                gout = torch.randn_like(out)
            out.backward(gout)
        res[route] = (out.detach(), xs.grad.clone(), _grads(stage))
    k, c = res["kernel"], res["composition"]
    _close("out", k[0], c[0])
    _close("dX", k[1], c[1])
    assert set(k[2]) == set(c[2]) and any("cnn_blocks.0.conv.kernel" in key for key in k[2])
    for key in k[2]:
        _close(key, k[2][key], c[2][key])


def test_spt_with_point_cnn_blocks(dev):
    from superpoint_transformer_amd import hotpath, nn as N
    from superpoint_transformer_amd import sparse as S
    from superpoint_transformer_amd.synthetic import make_nag
    small = make_nag("R", seed=3, device="cpu", sizes=(6000, 200, 80, 2500, 2000, 1))
    n0 = small.levels[0]["pos"].shape[0]
    coords, _ = R.random_cloud(n0, 24, 41)
    cfg = hotpath.spt64_config()
    pin = small.levels[0]["x"].shape[1]
    inj = 3 + 1
    cfg.update(point_cnn_blocks=True, point_cnn=[pin, 32, 32], point_cnn_kernel_size=3,
               point_cnn_dilation=1, point_cnn_norm=N.GraphNorm,
               point_cnn_activation=torch.nn.LeakyReLU(), point_mlp_on_cnn_feats=True,
               point_mlp=[32 + inj, 32, 64, 128])
    model = N.SPT(**cfg).to(dev)
    assert isinstance(model.first_stage.cnn_blocks, N.SparseCNN)

    class View:
        levels = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in lv.items()}
                  for lv in small.levels]
        num_clouds = 1

        def __getitem__(self, i):
            return self.levels[i]

    View.levels[0]["coords"] = coords.to(dev)
    res = {}
    for route in ("kernel", "composition"):
        model.zero_grad()
        with S.composition_only(route == "composition"):
            outs = model(View())
            sum(o.square().mean() for o in outs).backward()
        res[route] = ([o.detach() for o in outs], _grads(model))
    for a, b in zip(res["kernel"][0], res["composition"][0]):
        _close("stage output", a, b)
    gk, gc = res["kernel"][1], res["composition"][1]
    assert "first_stage.cnn_blocks.0.conv.kernel" in gk
    for key in ("first_stage.cnn_blocks.0.conv.kernel", "first_stage.cnn_blocks.1.conv.kernel",
                "first_stage.cnn_blocks.0.norm.weight"):
        _close(key, gk[key], gc[key])


def test_forward_and_backward_in_a_captured_graph(dev):
    from superpoint_transformer_amd import sparse as S
    coords, batch = R.random_cloud(500, 9, 51, batches=2)
    x, W, b, gout = _operands(500, 7, 32, 3, 9, integer=False)
    kmap = S.build_kernel_map(coords.to(dev), batch.to(dev), 3, 1)
    kmap.prepare_backward()
    xs, Ws, bs = (t.to(dev).requires_grad_() for t in (x, W, b))
    g = gout.to(dev)

    def step():
        out = S.sparse_conv3d(xs, Ws, kmap, bs)
        return (out,) + torch.autograd.grad(out, (xs, Ws, bs), g)

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    for name, e, c in zip(NAMES, eager, captured):
        assert torch.equal(e.view(torch.int32), c.detach().view(torch.int32)), name
    # other inputs in the same buffers: the replay follows them
    with torch.no_grad():
        xs.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize(dev)
    again = [t.detach().clone() for t in step()]
    for name, e, c in zip(NAMES, again, captured):
        assert torch.equal(e.view(torch.int32), c.detach().view(torch.int32)), name
