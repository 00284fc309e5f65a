"""CPU suite of the sparse convolution: the torch composition of ``sparse.py``
against the float64 dense twin, the offset order, the module surface of ``nn/sparse.py``, the two
transforms, the torchsparse import names and every refusal.  No GPU."""
import sys

import pytest
import torch

import sparse_conv_reference as R


def _case(n, ci, co, K, d, seed, batches=1, bias=True, dtype=torch.float64):
    coords, batch = R.random_cloud(n, 7, seed, batches)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, generator=g, dtype=dtype)
    shape = (K ** 3, ci, co) if K > 1 else (ci, co)
    W = torch.randn(shape, generator=g, dtype=dtype)
    b = torch.randn(co, generator=g, dtype=dtype) if bias else None
    gout = torch.randn(n, co, generator=g, dtype=dtype)
    return coords, batch, x, W, b, gout


def test_kernel_offsets_follow_the_formula():
    from superpoint_transformer_amd import sparse as S
    for K in (1, 3, 5, 7):
        for d in (1, 2, 3):
            off = S.kernel_offsets(K, d)
            assert off.shape == (K ** 3, 3) and off.dtype == torch.int64
            r = K // 2
            for o, (dx, dy, dz) in enumerate(off.tolist()):
                assert dx % d == 0 and dy % d == 0 and dz % d == 0
                assert o == ((dz // d + r) * K + (dy // d + r)) * K + (dx // d + r)
    # x fastest, the centre in the middle, the mirrored offset at K^3 - 1 - o
    off = S.kernel_offsets(3, 1)
    assert off[0].tolist() == [-1, -1, -1] and off[1].tolist() == [0, -1, -1]
    assert off[13].tolist() == [0, 0, 0]
    assert torch.equal(off.flip(0), -off)


@pytest.mark.parametrize("K,d", [(1, 1), (3, 1), (3, 2), (5, 1), (7, 1), (7, 2)])
def test_map_equals_the_brute_force_pairs(K, d):
    from superpoint_transformer_amd import sparse as S
    coords, batch = R.random_cloud(120, 7, K * 10 + d, batches=2)
    kmap = S.build_kernel_map(coords, batch, K, d)
    assert R.map_triples(kmap) == sorted(R.pairs_dense(coords, batch, K, d))
    assert kmap.rowptr[-1].item() == kmap.num_pairs and kmap.rowptr.numel() == 121
    perm, optr = kmap.by_offset_torch()
    assert torch.equal(kmap.off[perm].long(), torch.sort(kmap.off.long()).values)
    assert optr[-1].item() == kmap.num_pairs


@pytest.mark.parametrize("K,d", [(1, 1), (3, 1), (3, 2), (7, 1)])
@pytest.mark.parametrize("ci,co", [(1, 16), (3, 32), (7, 5)])
def test_cpu_route_against_the_twin(K, d, ci, co):
    from superpoint_transformer_amd import sparse as S
    coords, batch, x, W, b, gout = _case(90, ci, co, K, d, seed=K + d + ci, batches=2)
    kmap = S.build_kernel_map(coords, batch, K, d)
    xs, Ws, bs = x.clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()
    out = S.sparse_conv3d(xs, Ws, kmap, bs)
    (out * gout).sum().backward()
    want = R.conv_with_grads(x, W, coords, batch, K, d, b, gout)
    for got, ref in zip((out.detach(), xs.grad, Ws.grad, bs.grad), want):
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_cpu_route_without_bias_and_float_coords():
    from superpoint_transformer_amd import sparse as S
    coords, batch, x, W, _, _ = _case(60, 4, 16, 3, 1, seed=5, bias=False)
    a = S.sparse_conv3d(x, W, S.build_kernel_map(coords, None, 3, 1))
    b = S.sparse_conv3d(x, W, S.build_kernel_map(coords.double() - 3.0, None, 3, 1))
    assert torch.equal(a, b)
    assert (a - R.conv_dense(x, W, coords, None, 3, 1)).abs().max().item() < 1e-12


def test_negative_coordinates_and_batches_do_not_mix():
    from superpoint_transformer_amd import sparse as S
    coords, _ = R.random_cloud(80, 6, 9)
    shifted = coords - 40
    m0, m1 = S.build_kernel_map(coords, None, 3, 1), S.build_kernel_map(shifted, None, 3, 1)
    assert R.map_triples(m0) == R.map_triples(m1)
    both = torch.cat([coords, coords])
    batch = torch.cat([torch.zeros(80, dtype=torch.long), torch.ones(80, dtype=torch.long)])
    m2 = S.build_kernel_map(both, batch, 3, 1)
    row, nbr = m2.row.long(), m2.nbr.long()
    assert torch.equal(batch[row], batch[nbr]) and m2.num_pairs == 2 * m0.num_pairs


@pytest.mark.parametrize("K,d", [(3, 1), (3, 2), (7, 1)])
@pytest.mark.parametrize("pow2", [False, True])
def test_aliasing_traps(K, d, pow2):
    from superpoint_transformer_amd import sparse as S
    for coords, batch, (i, j) in R.aliasing_traps(K, d, pow2):
        kmap = S.build_kernel_map(coords, batch, K, d)
        pairs = {(a, c) for a, _, c in R.map_triples(kmap)}
        assert (i, j) not in pairs and (j, i) not in pairs
        assert R.map_triples(kmap) == sorted(R.pairs_dense(coords, batch, K, d))


def test_refusals():
    from superpoint_transformer_amd import sparse as S
    from superpoint_transformer_amd.nn import sparse as NS
    coords, _ = R.random_cloud(20, 5, 0)
    with pytest.raises(ValueError, match="even kernel"):
        S.build_kernel_map(coords, None, 2, 1)
    with pytest.raises(ValueError, match="even kernel"):
        S.kernel_offsets(4)
    with pytest.raises(NotImplementedError, match="stride"):
        S.build_kernel_map(coords, None, 3, 1, stride=2)
    with pytest.raises(NotImplementedError, match="stride"):
        NS.Conv3d(3, 16, 3, stride=2)
    with pytest.raises(NotImplementedError, match="transposed"):
        S.build_kernel_map(coords, None, 3, 1, transposed=True)
    with pytest.raises(NotImplementedError, match="transposed"):
        NS.Conv3d(3, 16, 3, transposed=True)
    with pytest.raises(ValueError, match="duplicate"):
        S.build_kernel_map(torch.cat([coords, coords[:1]]), None, 3, 1)
    with pytest.raises(ValueError, match="non-integer"):
        S.build_kernel_map(coords.float() + 0.25, None, 3, 1)
    with pytest.raises(ValueError, match="non-integer"):
        S.build_kernel_map(torch.tensor([[0.0, float("nan"), 0.0]]), None, 3, 1)
    far = torch.tensor([[0, 0, 0], [2 ** 30, 2 ** 30, 2 ** 30]])
    with pytest.raises(ValueError, match="bits"):
        S.build_kernel_map(far, torch.tensor([0, 2 ** 20]), 3, 1)
    with pytest.raises(ValueError, match="2\\^31"):
        S._refuse(0, 2 ** 31)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        S.build_kernel_map(coords[:, :2], None, 3, 1)
    with pytest.raises(ValueError, match="no active voxel"):
        S.build_kernel_map(coords[:0], None, 3, 1)
    kmap = S.build_kernel_map(coords, None, 3, 1)
    with pytest.raises(ValueError, match="weight"):
        S.sparse_conv3d(torch.zeros(20, 3), torch.zeros(26, 3, 16), kmap)
    with pytest.raises(ValueError, match="x must be"):
        S.sparse_conv3d(torch.zeros(19, 3), torch.zeros(27, 3, 16), kmap)


def test_sparse_cnn_state_dict_and_surface():
    from superpoint_transformer_amd.nn import GraphNorm
    from superpoint_transformer_amd.nn.sparse import LeakyReLU, ReLU, SiLU, SparseCNN
    cnn = SparseCNN([3, 32, 32, 32], 3, 1)
    sd = cnn.state_dict()
    want = {}
    for i, (a, b) in enumerate([(3, 32), (32, 32), (32, 32)]):
        want[f"{i}.conv.kernel"] = (27, a, b)
        for p in ("weight", "bias", "mean_scale"):
            want[f"{i}.norm.{p}"] = (32,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert cnn.out_dim == 32 and isinstance(cnn[0].norm, GraphNorm) and cnn[0].conv.bias is None
    big = SparseCNN([5, 32, 32, 32], [7, 3, 3], [1, 1, 1], activation="leakyrelu")
    assert tuple(big[0].conv.kernel.shape) == (343, 5, 32)
    assert tuple(big[1].conv.kernel.shape) == (27, 32, 32)
    assert isinstance(big[0].activation, LeakyReLU)
    one = SparseCNN([4, 16], 1, 1, norm=None)
    assert tuple(one[0].conv.kernel.shape) == (4, 16) and tuple(one[0].conv.bias.shape) == (16,)
    assert float(one[0].conv.bias.detach().abs().max()) == 0.0
    # _conv_init: xavier uniform with the leaky-relu gain on (out, in, volume)
    k = cnn[1].conv.kernel.detach()
    bound = torch.nn.init.calculate_gain("leaky_relu") * (6.0 / (32 * 27 + 32 * 27)) ** 0.5
    assert float(k.abs().max()) <= bound and float(k.abs().max()) > 0.9 * bound
    # check_type, activations, residuals, freeze
    assert cnn.check_type(3) == [3, 3, 3] and cnn.check_type([7, 3, 3]) == [7, 3, 3]
    with pytest.raises(AssertionError):
        cnn.check_type([3, 3])
    with pytest.raises(ValueError):
        cnn.check_type("3")
    assert isinstance(SparseCNN([3, 16], 3, 1, activation=torch.nn.SiLU())[0].activation, SiLU)
    assert isinstance(SparseCNN([3, 16], 3, 1, activation=torch.nn.ReLU())[0].activation, ReLU)
    act = SparseCNN([3, 16], 3, 1, activation=torch.nn.LeakyReLU(0.2))[0].activation
    assert isinstance(act, LeakyReLU) and act.negative_slope == 0.2
    with pytest.raises(ValueError, match="Invalid activation"):
        SparseCNN([3, 16], 3, 1, activation=torch.nn.Tanh())
    with pytest.raises(ValueError, match="Invalid activation"):
        SparseCNN([3, 16], 3, 1, activation="gelu")
    with pytest.raises(AssertionError):
        SparseCNN([3, 16, 16], 3, 1, residual=[True, True])
    with pytest.raises(AssertionError):
        SparseCNN([3, 16, 16], 3, 1, global_residual=True)
    SparseCNN([16, 16, 16], 3, 1, residual=True, global_residual=True)
    last = SparseCNN([3, 16, 16], 3, 1, last_norm=False, last_activation=False)
    assert last[1].norm is None and last[1].activation is None and last[0].norm is not None
    with pytest.raises(NotImplementedError, match="index-based"):
        SparseCNN([3, 16], 3, 1, norm=torch.nn.BatchNorm1d)
    cnn.freeze()
    assert cnn.frozen and not any(p.requires_grad for p in cnn.parameters())
    cnn.unfreeze()
    assert not cnn.frozen and all(p.requires_grad for p in cnn.parameters())


def test_sparse_cnn_forward_on_the_cpu_route_shares_one_map():
    from superpoint_transformer_amd import sparse as S
    from superpoint_transformer_amd.nn.sparse import SparseCNN, SparseTensor
    torch.manual_seed(0)
    coords, batch = R.random_cloud(70, 6, 3, batches=2)
    cnn = SparseCNN([4, 16, 16, 16], 3, 1, norm=None, activation="relu", residual=[False, True, True])
    x = torch.randn(70, 4)
    st = SparseTensor(coords=torch.cat([batch.view(-1, 1), coords], 1).int(), feats=x)
    built = []
    real = S.build_kernel_map
    try:
        S.build_kernel_map = lambda *a, **k: built.append(1) or real(*a, **k)
        out = cnn(st)
    finally:
        S.build_kernel_map = real
    assert len(built) == 1 and out.F.shape == (70, 16) and out.C is st.C
    h = x.double()
    for blk in cnn:
        y = R.conv_dense(h, blk.conv.kernel.detach(), coords, batch, 3, 1, blk.conv.bias.detach())
        h = torch.relu(y + h if blk.residual else y)
    assert (out.F.double() - h).abs().max().item() < 1e-4


def test_pretrained_cnn_load_checkpoint(tmp_path):
    from superpoint_transformer_amd.nn import PointStage
    from superpoint_transformer_amd.transforms import PretrainedCNN

    def stage():
        return PointStage(None, cnn_blocks=True, cnn=[3, 16, 16], cnn_kernel_size=3, cnn_dilation=1,
                          cnn_norm=None, cnn_activation="relu", use_pos=False)

    torch.manual_seed(1)
    src, dst = stage(), stage()
    sd = {"net.first_stage." + k: v.clone() for k, v in src.state_dict().items()}
    sd["net.down_stages.0.whatever"] = torch.zeros(3)
    sd["net.first_stage.not_there"] = torch.zeros(2)
    path = tmp_path / "ckpt.pt"
    torch.save({"state_dict": sd}, path)
    assert not torch.equal(dst.cnn_blocks[0].conv.kernel, src.cnn_blocks[0].conv.kernel)
    out = PretrainedCNN.load_checkpoint(dst, str(path), "cpu")
    assert out is dst
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v)
    sd["net.first_stage.cnn_blocks.0.conv.kernel"] = torch.zeros(27, 3, 8)
    torch.save({"state_dict": sd}, path)
    with pytest.raises(ValueError, match="Shape mismatch"):
        PretrainedCNN.load_checkpoint(stage(), str(path), "cpu")
    with pytest.raises(AssertionError):
        PretrainedCNN.load_checkpoint(stage(), str(tmp_path / "missing.pt"), "cpu")
    with pytest.raises(AssertionError, match="partition_hf"):
        PretrainedCNN(stage(), str(path), partition_hf=None, device="cpu")


@pytest.mark.parametrize("with_batch", [False, True])
@pytest.mark.parametrize("allow_negative", [False, True])
def test_quantize_point_coordinates(with_batch, allow_negative):
    from superpoint_transformer_amd.data import NAG, Data
    from superpoint_transformer_amd.transforms import QuantizePointCoordinates
    g = torch.Generator().manual_seed(4)
    n = 400
    pos = (torch.rand(n, 3, generator=g) - 0.5) * 2.0
    batch = (torch.arange(n) >= 250).long() if with_batch else None
    # (one level: selecting below a partition relabels super_index, which runs on the device
    # only - tests/test_sparse_conv_gpu.py does that)
    d0 = Data(pos=pos, x=torch.randn(n, 2, generator=g))
    if with_batch:
        d0.batch = batch
    nag = NAG([d0])
    size = 0.2
    assert QuantizePointCoordinates(0)(nag) is nag
    out = QuantizePointCoordinates(size, allow_negative_coords=allow_negative)(nag)
    # the restatement: unique on the (batch, z, y, x) key, the LAST index of each voxel wins
    c = torch.round(pos / size).long()
    c0 = c - c.min(0).values
    ext = c0.max(0).values + 1
    key = ((batch if with_batch else torch.zeros(n, dtype=torch.long)) * ext[2] + c0[:, 2])
    key = (key * ext[1] + c0[:, 1]) * ext[0] + c0[:, 0]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    last = torch.zeros(uniq.numel(), dtype=torch.long)
    last.scatter_reduce_(0, inv, torch.arange(n), "amax", include_self=False)
    assert torch.equal(out[0].pos, pos[last])
    want = torch.round(pos / size)[last]
    if not allow_negative:
        want = want - want.min(0, keepdim=True).values
        assert float(out[0].coords.min()) == 0.0
    assert torch.equal(out[0].coords, want) and out[0].coords.is_floating_point()
    assert out[0].num_nodes == uniq.numel() < n


def test_torchsparse_import_names():
    from superpoint_transformer_amd import shims
    from superpoint_transformer_amd.nn import sparse as NS
    saved = {k: sys.modules.get(k) for k in ("torchsparse", "torchsparse.nn")}
    try:
        assert "torchsparse" in shims.install(force=True)
        from torchsparse import SparseTensor
        from torchsparse import nn as spnn
        import torchsparse.nn as spnn2
        assert spnn is spnn2 and SparseTensor is NS.SparseTensor
        assert spnn.Conv3d is NS.Conv3d and spnn.ReLU is NS.ReLU
        assert spnn.LeakyReLU is NS.LeakyReLU and spnn.SiLU is NS.SiLU
        coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32)
        a = SparseTensor(coords=coords, feats=torch.ones(2, 3))
        b = a + a
        assert torch.equal(b.F, 2 * torch.ones(2, 3)) and b.C is a.C
        conv = spnn.Conv3d(3, 16, kernel_size=3, stride=1, dilation=1, bias=True)
        y = spnn.LeakyReLU(0.1)(conv(a))
        assert y.F.shape == (2, 16) and y._maps is a._maps and len(a._maps) == 1
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


REF = "/root/reference"


@pytest.mark.skipif(not __import__("os").path.isdir(REF),
                    reason="reference tree only exists in the build container")
def test_reference_sparse_cnn_constructs_and_runs_on_the_shim():
    """The reference's own src/nn/sparse.py, imported unchanged on the torchsparse shim: same
    state-dict keys and shapes as ``nn.sparse.SparseCNN``, and the same output from the same
    parameters (CPU route; no norm: GraphNorm runs on the device only)."""
    import importlib
    import os
    import types
    from superpoint_transformer_amd import shims
    from superpoint_transformer_amd.nn import sparse as NS
    keep = ("src", "torchsparse", "omegaconf", "numba", "git")
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in keep}
    try:
        shims.install(force=True)

        def pkg(name, path=None):
            m = types.ModuleType(name)
            m.__path__ = [path] if path else []
            sys.modules[name] = m
            return m

        if "omegaconf" not in sys.modules:
            try:
                importlib.import_module("omegaconf")
            except ImportError:
                oc = types.ModuleType("omegaconf")
                oc.ListConfig = type("ListConfig", (list,), {})
                sys.modules["omegaconf"] = oc
        src = pkg("src", os.path.join(REF, "src"))
        src.is_debug_enabled = lambda: False
        pkg("src.nn", os.path.join(REF, "src", "nn"))
        pkg("src.utils", os.path.join(REF, "src", "utils"))
        pkg("src.dependencies")
        pkg("src.dependencies.FRNN").frnn = sys.modules["src.dependencies.FRNN.frnn"]
        numba = types.ModuleType("numba")
        numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
        sys.modules.setdefault("numba", numba)
        sys.modules.setdefault("git", types.ModuleType("git"))
        U = sys.modules["src.utils"]
        for sub in ("dict", "parameter", "version", "nn", "tensor", "sparse", "edge", "scatter",
                    "neighbors", "geometry", "graph"):
            m = importlib.import_module(f"src.utils.{sub}")
            for k in getattr(m, "__all__", []):
                setattr(U, k, getattr(m, k))
        theirs_mod = importlib.import_module("src.nn.sparse")
        assert theirs_mod.SparseTensor is NS.SparseTensor
        for args, kw in ((([3, 32, 32, 32], 3, 1), {}),
                         (([5, 32, 32, 32], [7, 3, 3], 1), dict(activation="leakyrelu")),
                         (([4, 16, 16], 3, 1), dict(norm=None, residual=[False, True]))):
            theirs, ours = theirs_mod.SparseCNN(*args, **kw), NS.SparseCNN(*args, **kw)
            assert {k: tuple(v.shape) for k, v in theirs.state_dict().items()} == \
                   {k: tuple(v.shape) for k, v in ours.state_dict().items()}
        ours.load_state_dict(theirs.state_dict())
        coords, batch = R.random_cloud(50, 5, 2, batches=2)
        c4 = torch.cat([batch.view(-1, 1), coords], 1).int()
        x = torch.randn(50, 4)
        a = theirs(NS.SparseTensor(coords=c4, feats=x)).F
        b = ours(NS.SparseTensor(coords=c4, feats=x)).F
        assert torch.equal(a, b) and a.shape == (50, 16)
    finally:
        for k in [k for k in sys.modules if k.split(".")[0] in keep]:
            del sys.modules[k]
        sys.modules.update(saved)
