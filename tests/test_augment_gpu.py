"""GPU suite of the augmentation kernels (csrc/augment.hip) and of the transform classes on a
device NAG: fixture parity, the random stream at n = 2**20, bitwise independence of the route a
row takes, fused == stepwise, guarded buffers, no host read."""
import numpy as np
import pytest
import torch

import augment_reference as AR
import test_augment_reference_cpu as C
from guarded import GuardedArena
from superpoint_transformer_amd import augment as A
from superpoint_transformer_amd import transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1 << 20


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
def test_kernels_reproduce_fixture():
    """The classes' ``apply`` on device tensors with the fixture's recorded draws: exact where
    the map is exact, within MARGIN x REFERENCE_DEVIATION where it is bounded."""
    report = {}
    C.run_classes_against_fixture(DEV, report)
    for (case, name), dev in sorted(report.items()):
        print(f"kernel vs fixture  {case:15s} {name:14s} {dev:.4e}  "
              f"(bound {AR.MARGIN * AR.REFERENCE_DEVIATION[name]:.4e})")
    assert {n for _, n in report} == set(AR.REFERENCE_DEVIATION)
    C.run_stream_classes(DEV)


@pytest.mark.parametrize("sigma,trunc", list(AR.NOISE_DEVIATION))
def test_noise_stream(sigma, trunc):
    seed = 12345678901234567
    z = A.jitter_(torch.zeros(N, device=DEV), sigma, trunc, seed=seed).cpu().numpy().astype(np.float64)
    ref = AR.noise(seed, np.arange(N), sigma, trunc)
    dev = np.abs(z - ref).max() / sigma
    bound = AR.MARGIN * AR.NOISE_DEVIATION[(sigma, trunc)]
    ks, lag = AR.ks_distance(z, sigma, trunc), abs(AR.lag1(z))
    print(f"kernel noise vs f64  sigma {sigma} trunc {trunc}: {dev:.3e} sigma (bound {bound:.3e}), "
          f"KS {ks:.5f}, lag-1 {lag:.5f}, max |z| {np.abs(z).max() / sigma:.3f} sigma")
    assert np.isfinite(z).all()
    assert dev <= bound
    if trunc > 0:
        assert np.abs(z).max() <= np.float32(trunc)
    assert ks <= np.sqrt(np.log(2 / 1e-9) / (2 * N))
    assert lag <= 6 / np.sqrt(N)
    other = A.jitter_(torch.zeros(N, device=DEV), sigma, trunc, seed=seed + 1).cpu().numpy()
    assert (other != z.astype(np.float32)).mean() > 0.99


@pytest.mark.parametrize("p", [0.3, 0.5])
def test_row_decisions_stream(p):
    for seed in (0, 12345678901234567):
        x = A.dropout_(torch.ones(N, 1, device=DEV), p_rows=p, seed_rows=seed)
        dropped = (x[:, 0] == 0).cpu().numpy()
        assert np.array_equal(dropped, AR.decisions(seed, np.arange(N), p))
        off = abs(dropped.sum() - N * p) / np.sqrt(N * p * (1 - p))
        print(f"rows dropped p {p} seed {seed}: {dropped.sum()} ({off:.2f} sigma off)")
        assert off <= 6
    a = A.dropout_(torch.ones(N, 1, device=DEV), p_rows=p, seed_rows=1)
    assert not torch.equal(a, x)


# ---------------------------------------------------------------------------
# route independence
# ---------------------------------------------------------------------------
ROWS = (1, 3, 4, 5, 63, 65, 257, 100_003)
R9 = torch.tensor(AR.rodrigues([0.3, -0.2, 1.0], 77.0), dtype=torch.float32)
S3 = torch.tensor([1.1, 0.9, 1.05])
JIT = (0.02, 0.04, 99)


def calls(c):
    """[(name, fn(x, out))] of the kernels that take c-column rows, every step switched on."""
    out = [("features", lambda x, out: A.features_(
        x, jitter=JIT, col_mask=(0b1000101 & ((1 << c) - 1)) if c > 1 else 0, p_rows=0.3, seed_rows=5,
        out=out))]
    if c == 3:
        rng6 = torch.tensor([-0.2, -0.1, 0.0, 1.3, 1.2, 1.1], device=DEV)
        out += [("pos", lambda x, out: A.geometry_(x, A.POS, jitter=JIT, R=R9, scale=S3, flip_axis=1, out=out)),
                ("normal", lambda x, out: A.geometry_(x, A.NORMAL, R=R9, scale=S3, flip_axis=2, out=out)),
                ("color", lambda x, out: A.color_(x, jitter=JIT, contrast=0.4, out=out, range6=rng6))]
    if c == 7:
        out += [("edge7", lambda x, out: A.geometry_(x, A.EDGE7, R=R9, scale=S3, flip_axis=0, out=out))]
    return out


@pytest.mark.parametrize("c", [1, 3, 7, 18])
def test_route_independence(c):
    gen = torch.Generator().manual_seed(c)
    for n in ROWS:
        src = torch.randn(n + 13, c, generator=gen).to(DEV)
        for name, fn in calls(c):
            base = fn(src[:n].clone(), None)                         # dense, aligned, in place
            # out != in
            x = src[:n].clone()
            out = torch.full_like(x, 7.0)
            fn(x, out)
            assert same(out, base) and same(x, src[:n]), (name, n, "out != in")
            # column slice of a wider tensor, in place and into another wide tensor
            wide = torch.full((n, c + 5), 3.0, device=DEV)
            wide[:, 2:2 + c] = src[:n]
            fn(wide[:, 2:2 + c], None)
            assert same(wide[:, 2:2 + c], base), (name, n, "slice")
            assert (wide[:, :2] == 3).all() and (wide[:, 2 + c:] == 3).all(), (name, n, "slice border")
            wide2 = torch.full((n, c + 4), 3.0, device=DEV)
            fn(src[:n].clone(), wide2[:, 1:1 + c])
            assert same(wide2[:, 1:1 + c], base) and (wide2[:, 0] == 3).all() and (wide2[:, 1 + c:] == 3).all()
            # unaligned base (4 bytes past a 16-byte boundary), dense
            flat = torch.zeros(n * c + 1, device=DEV)
            un = flat[1:].view(n, c)
            assert un.data_ptr() % 16 == 4
            un.copy_(src[:n])
            fn(un, None)
            assert same(un, base), (name, n, "unaligned")
            # prefix of a longer call
            longer = fn(src.clone(), None)
            assert same(longer[:n], base), (name, n, "prefix")


def test_color_range_routes_and_reproducible():
    gen = torch.Generator().manual_seed(0)
    for n in ROWS:
        c = torch.rand(n, 3, generator=gen).to(DEV)
        r = A.color_range(c, jitter=JIT)
        want = torch.from_numpy(AR.jitter(c.cpu().numpy(), JIT[2], JIT[0], JIT[1]))
        lo, hi = want.min(0).values, want.max(0).values
        got = r.cpu().double()
        assert (got[:3] - lo).abs().max() < 1e-6 and (got[3:] - hi).abs().max() < 1e-6
        wide = torch.zeros(n, 8, device=DEV)
        wide[:, 4:7] = c
        assert same(A.color_range(wide[:, 4:7], jitter=JIT), r)
        flat = torch.zeros(n * 3 + 1, device=DEV)
        flat[1:] = c.view(-1)
        assert same(A.color_range(flat[1:].view(n, 3), jitter=JIT), r)
        assert same(A.color_range(c, jitter=JIT), r)
        # the colour kernel's jittered values are the ones the range was taken of
        j = A.color_(c.clone(), jitter=JIT)
        assert same(torch.cat((j.min(0).values, j.max(0).values)), r)
    # without jitter: the plain range, signed zeros and negatives ordered
    c = torch.tensor([[-0.0, -2.0, 5.0], [0.0, -3.0, -1.0], [-1.0, -2.5, 0.0]], device=DEV)
    assert A.color_range(c).tolist() == [-1.0, -3.0, -1.0, 0.0, -2.0, 5.0]
    c[1, 1] = float("nan")
    r = A.color_range(c)
    assert torch.isnan(r[[1, 4]]).all() and r[[0, 2, 3, 5]].tolist() == [-1.0, -1.0, 0.0, 5.0]


def test_empty_tensors_make_no_launch():
    before = dict(A.LAUNCHES)
    e3, e7 = torch.empty(0, 3, device=DEV), torch.empty(0, 7, device=DEV)
    A.features_(e7, jitter=JIT, col_mask=1, p_rows=0.5, seed_rows=1)
    A.geometry_(e3, A.POS, jitter=JIT, R=R9, scale=S3, flip_axis=0)
    A.geometry_(e7, A.EDGE7, R=R9)
    A.color_(e3, jitter=JIT, contrast=0.5, drop=True)
    assert A.LAUNCHES == before


# ---------------------------------------------------------------------------
def test_fused_equals_stepwise_and_repeats():
    first = C.fused_and_stepwise(DEV)
    for name, a, b in first:
        C.assert_same_nags(a, b, name)
    for (name, a, _), (_, a2, _) in zip(first, C.fused_and_stepwise(DEV)):
        C.assert_same_nags(a, a2, name + " repeated")


def test_fused_launch_counts():
    """One launch per tensor touched, plus one range launch per contrasted colour tensor."""
    nag = C.train_nag(DEV)
    before = A.LAUNCHES["kernels"]
    torch.manual_seed(1)
    T.GeometricAugmentation(pos_jitter=0.03, trunc=0.03, phi=60, theta=180, delta=0.2, flip_p=1.0)(nag)
    touched = sum(1 for i in range(3) for k in ("pos", "normal", "mean_normal", "edge_attr")
                  if nag[i].get(k) is not None)
    assert A.LAUNCHES["kernels"] - before == touched == 11
    nag = C.train_nag(DEV, 18)
    before = A.LAUNCHES["kernels"]
    T.FeatureAugmentation(key=["linearity", "edge_attr"], sigma=0.01, trunc=0.02, p_columns=0.3, p_rows=0.3)(nag)
    assert A.LAUNCHES["kernels"] - before == 5
    nag = C.train_nag(DEV)
    before = A.LAUNCHES["kernels"]
    aug = T.ColorAugmentation(sigma=0.05, trunc=0.1, p_contrast=0.7, p_drop=0.3)
    params = aug.draw(nag)
    aug.apply(nag, params)
    touched = set(params["jitter"]) | set(params["contrast"]) | set(params["drop"])
    assert A.LAUNCHES["kernels"] - before == len(touched) + len(params["contrast"])


# ---------------------------------------------------------------------------
def test_guarded_buffers():
    arena = GuardedArena(DEV, guard=1 << 16)
    gen = torch.Generator().manual_seed(3)
    for n in (5, 257, 1003):
        for c in (1, 3, 7, 18):
            for name, fn in calls(c):
                x = arena.take(4 * n * c, torch.float32, (n, c))
                x.copy_(torch.randn(n, c, generator=gen))
                out = arena.take(4 * n * c, torch.float32, (n, c))
                fn(x, out)
                fn(x, None)
                # strided: the last row of the slice ends with the buffer
                ld = c + 3
                wide = arena.take(4 * (n * ld - 3), torch.float32)
                wide.fill_(3.0)
                view = wide.as_strided((n, c), (ld, 1))
                fn(view, None)
                rest = wide.as_strided((n - 1, 3), (ld, 1), storage_offset=wide.storage_offset() + c)
                assert (rest == 3).all(), (name, n, c)
        col = arena.take(4 * n * 3, torch.float32, (n, 3))
        col.copy_(torch.rand(n, 3, generator=gen))
        r6 = arena.take(24, torch.float32, (6,))
        A.color_range(col, jitter=JIT, out=r6)
        A.color_(col, jitter=JIT, contrast=0.3, drop=False, range6=r6)
    arena.check()


def test_train_block_makes_no_host_read():
    """The default train block (three fused classes on three levels) under
    torch.cuda.set_sync_debug_mode('error')."""
    nag = C.train_nag(DEV, 7)
    feat = C.train_nag(DEV, 18)
    block = [T.GeometricAugmentation(pos_jitter=0.01, trunc=0.02, phi=5, theta=180, delta=0.2),
             T.ColorAugmentation(sigma=0.05, trunc=0.1, p_contrast=1.0, p_drop=0.5)]
    fblock = [T.FeatureAugmentation(key=["linearity", "edge_attr"], sigma=0.01, trunc=0.02,
                                    p_columns=0.3, p_rows=0.3)]
    torch.cuda.synchronize()
    torch.manual_seed(0)
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                       # the mode is honoured: a host read raises
        for t in block:
            t(nag)
        for t in fblock:
            t(feat)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not C.same_bits(nag[0]["pos"].cpu().numpy(), C.train_nag()[0]["pos"].numpy())
