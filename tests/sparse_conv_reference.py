"""Float64 twin of the stride-1 sparse convolution, written from the specification
alone: scatter the features into a dense ``[B, C, Z, Y, X]`` grid, run
``torch.nn.functional.conv3d`` with ``padding = r d``, ``dilation = d`` and
``w[co, ci, dz, dy, dx] = W[o]``, read the result at the active sites.  conv3d is a
cross-correlation, so ``out[z, y, x] = sum w[dz, dy, dx] in[z + d (dz - r), ...]``: the
specification's sign.  Gradients come from autograd on the same graph.

Also the cases the device tests share (coordinates only; small and deterministic)."""
import numpy as np
import torch


def dense_weight(W, K):
    """[K^3, Ci, Co] (or [Ci, Co] for K = 1) -> [Co, Ci, K, K, K] with o = (dz K + dy) K + dx."""
    W = W.reshape(K ** 3, W.shape[-2], W.shape[-1])
    return W.reshape(K, K, K, W.shape[1], W.shape[2]).permute(4, 3, 0, 1, 2)


def conv_dense(x, W, coords, batch=None, K=3, d=1, bias=None, dtype=torch.float64):
    """The twin's forward: every argument a CPU tensor; x / W / bias may require grad (dtype)."""
    c = coords.long()
    n = c.shape[0]
    b = torch.zeros(n, dtype=torch.long) if batch is None else batch.long()
    b = b - b.min()
    c = c - c.min(dim=0).values
    X, Y, Z = (int(v) + 1 for v in c.max(dim=0).values)
    B = int(b.max()) + 1
    ci = x.shape[1]
    grid = torch.zeros(B, Z, Y, X, ci, dtype=dtype)
    grid = grid.index_put((b, c[:, 2], c[:, 1], c[:, 0]), x.to(dtype))
    r = K // 2
    out = torch.nn.functional.conv3d(grid.permute(0, 4, 1, 2, 3), dense_weight(W.to(dtype), K),
                                     None if bias is None else bias.to(dtype), padding=r * d,
                                     dilation=d)
    return out.permute(0, 2, 3, 4, 1)[b, c[:, 2], c[:, 1], c[:, 0]]


def conv_with_grads(x, W, coords, batch, K, d, bias, gout, dtype=torch.float64):
    """(out, dX, dW, dbias) of the twin in ``dtype`` for the upstream gradient ``gout``."""
    xs = x.detach().to(dtype).requires_grad_()
    Ws = W.detach().to(dtype).requires_grad_()
    bs = None if bias is None else bias.detach().to(dtype).requires_grad_()
    out = conv_dense(xs, Ws, coords, batch, K, d, bs, dtype)
    (out * gout.to(dtype)).sum().backward()
    return out.detach(), xs.grad, Ws.grad, None if bs is None else bs.grad


def pairs_dense(coords, batch, K, d):
    """The kernel map by brute force, as a sorted list of (i, o, j)."""
    c = coords.long().tolist()
    b = [0] * len(c) if batch is None else batch.long().tolist()
    where = {(bb, *cc): i for i, (bb, cc) in enumerate(zip(b, c))}
    r = K // 2
    out = []
    for i, (bb, (x, y, z)) in enumerate(zip(b, c)):
        for dz in range(-r, r + 1):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    j = where.get((bb, x + d * dx, y + d * dy, z + d * dz))
                    if j is not None:
                        out.append((i, ((dz + r) * K + (dy + r)) * K + (dx + r), j))
    return out


def map_triples(kmap):
    return list(zip(kmap.row.tolist(), kmap.off.tolist(), kmap.nbr.tolist()))


# ---- coordinates --------------------------------------------------------------------------------
def random_cloud(n, extent, seed, batches=1):
    """n distinct voxels of [0, extent)^3 per call (over ``batches`` items), shuffled."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(batches * extent ** 3, size=n, replace=False)
    b, rem = np.divmod(cells, extent ** 3)
    z, rem = np.divmod(rem, extent ** 2)
    y, x = np.divmod(rem, extent)
    coords = torch.from_numpy(np.stack([x, y, z], 1).astype(np.int64))
    batch = torch.from_numpy(b.astype(np.int64)) if batches > 1 else None
    return coords, batch


def full_block(side=9):
    ax = torch.arange(side)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)


def plane_and_shell(seed=0, side=150, radius=40):
    """A noisy plane (item 0) and a sphere shell (item 1): about 50 000 distinct voxels."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    zs = np.rint(rng.normal(0.0, 0.7, xs.shape)).astype(np.int64)
    plane = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)
    g = np.arange(-radius - 1, radius + 2)
    gx, gy, gz = np.meshgrid(g, g, g, indexing="ij")
    rad = np.sqrt(gx ** 2 + gy ** 2 + gz ** 2)
    on = np.abs(rad - radius) < 0.6
    shell = np.stack([gx[on], gy[on], gz[on]], 1)
    coords = np.concatenate([plane, shell]).astype(np.int64)
    batch = np.concatenate([np.zeros(len(plane), np.int64), np.ones(len(shell), np.int64)])
    perm = rng.permutation(len(coords))
    return torch.from_numpy(coords[perm]), torch.from_numpy(batch[perm])


def aliasing_traps(K, d, power_of_two):
    """[(coords, batch, (i, j))]: voxel i at the maximum of an axis and voxel j at the minimum of
    the next row / slab / batch item, placed so that an unpadded key of ``max + 1`` would equal
    j's key.  The pair (i, j) must be absent.  ``power_of_two``: extents of exactly 2^k."""
    r = K // 2
    ext = 8
    while ext < 4 * r * d + 2:                               # far beyond reach along the axis
        ext *= 2
    if not power_of_two:
        ext -= 2
    hi = ext - 1
    traps = []
    # x overflow -> next y row; y overflow -> next z slab; z overflow -> next batch item
    frame = [[0, 0, 0], [hi, hi, hi]]                        # pins the bounds of every axis
    for axis in range(3):
        a, b = [1, 1, 1], [1, 1, 1]
        a[axis] = hi
        b[axis] = 0
        if axis < 2:
            b[axis + 1] = 2
        coords = torch.tensor(frame + [a, b] + frame, dtype=torch.int64)
        batch = torch.tensor([0, 0, 0, 0 if axis < 2 else 1, 1, 1], dtype=torch.int64)
        traps.append((coords, batch, (2, 3)))
        # the same one step further out: reachable at distance r d as well
        if r * d > 1:
            a2 = list(a)
            a2[axis] = hi - (r * d - 1)
            coords2 = torch.tensor(frame + [a2, b] + frame, dtype=torch.int64)
            traps.append((coords2, batch.clone(), (2, 3)))
    return traps
