"""The augmentation block of the training chain at batch (T) and scene (S) size, three legs on
the device:

  torch     the reference's composition restated in torch: trunc_normal_ per key, matmul per
            tensor for the rotation, index_fill_ after torch.where(...)[0] for the dropouts, and
            a host read at every decision (``if torch.rand(1, device=...) < p``)
  stepwise  the eight transform classes of transforms.py, one after the other
  fused     GeometricAugmentation, FeatureAugmentation (point features, edge_attr),
            ColorAugmentation

    python tools/augment_bench.py [T|S] [--leg all|torch|stepwise|fused] [--reps N]

The levels look as they do after the sampling transforms: N0 / N1 / N2 nodes, ``pos``,
``normal``, ``rgb`` and five 1-column point features per level; the geometric group sees the
trimmed 7-column ``edge_attr`` (E / 2 rows), the feature group the 18-column one (E rows).
Settings are the S3DIS ones (pos_jitter 0.03 / voxel 0.03, tilt 5 / 180, scale 0.2, flip 0.5,
feature jitter 0.01, column drop 0.3, row drop 0, rgb jitter 0.03, auto-contrast 0.5, drop 0.2).

Per leg: device time, host wall time, kernel launches of this package (``augment.LAUNCHES``; a
range launch also makes two 12-byte fills), and, counted with a dispatch mode on one extra call,
the torch operators that compute on the device and the host reads (``.item()`` / ``bool()`` of a
device tensor, ``nonzero``).
"""
import argparse
import os
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import augment as A  # noqa: E402
from superpoint_transformer_amd import transforms as T  # noqa: E402
from superpoint_transformer_amd.data import NAG, Data  # noqa: E402
from superpoint_transformer_amd.synthetic import SCENES  # noqa: E402

POINT_KEYS = ["linearity", "planarity", "scattering", "verticality", "elevation"]
CFG = dict(pos_jitter=0.03, voxel=0.03, phi=5, theta=180, delta=0.2, flip_p=0.5, feat_jitter=0.01,
           feat_drop=0.3, edge_jitter=0.01, edge_drop=0.3, row_drop=0.0, rgb_jitter=0.03,
           contrast=0.5, rgb_drop=0.2)

_FREE = ("view", "empty", "slice", "select", "transpose", "expand", "unsqueeze", "squeeze",
         "as_strided", "detach", "alias", "reshape", "permute", "t.", "_to_copy", "lift_fresh")


class Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops, self.reads = 0, 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        on_device = any(torch.is_tensor(a) and a.is_cuda for a in list(args) + list((kwargs or {}).values()))
        if "_local_scalar_dense" in name or "nonzero" in name or "is_nonzero" in name:
            self.reads += on_device
        elif on_device and not any(f in name for f in _FREE):
            self.ops += 1
        return func(*args, **(kwargs or {}))


def timed(fn, reps, settle=0.3):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    time.sleep(settle)
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
    ev.sort(), wall.sort()
    return ev[len(ev) // 2], ev[0], wall[len(wall) // 2]


def make_nag(scene, dev, edge_cols):
    n0, n1, n2, e1, e2, _ = SCENES[scene]
    gen = torch.Generator(device=dev).manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=gen, device=dev)  # noqa: E731
    levels = []
    for n, e in ((n0, 0), (n1, e1), (n2, e2)):
        d = Data(pos=r(n, 3) * 4, normal=torch.nn.functional.normalize(r(n, 3).abs()),
                 rgb=torch.rand(n, 3, generator=gen, device=dev))
        for k in POINT_KEYS:
            d[k] = torch.rand(n, 1, generator=gen, device=dev)
        if e:
            d.edge_attr = r(e // 2 if edge_cols == 7 else e, edge_cols)
        levels.append(d)
    return NAG(levels)


# ---- the reference's composition, restated --------------------------------------------------
def t_jitter(nag, keys, sigma, trunc):
    for i in range(nag.num_levels):
        for k in keys:
            a = nag[i].get(k)
            if a is not None:
                a += torch.nn.init.trunc_normal_(torch.empty_like(a), mean=0., std=sigma, a=-trunc, b=trunc)


def t_dropout(a, p, dim):
    idx = torch.where(torch.rand(a.shape[dim], device=a.device) < p)[0]
    return a.index_fill_(dim, idx, 0)


def t_up(nrm):
    nrm[nrm[:, 2] < 0] *= -1
    return nrm


def t_geometry(nag, c):
    dev = nag.device
    t_jitter(nag, ["pos"], c["pos_jitter"], c["voxel"])
    sigma = c["phi"] / 180. * torch.pi / 3
    xy = torch.distributions.MultivariateNormal(torch.zeros(2, device=dev), torch.eye(2, device=dev) * sigma).sample()
    axis = torch.cat((xy, torch.ones(1, device=dev)))
    axis = axis / axis.norm()
    theta = torch.rand(1, device=dev) * 2 * c["theta"] - c["theta"]
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], device=dev)
    t = torch.tensor([theta / 180. * torch.pi], device=dev)
    R = torch.eye(3, device=dev) + torch.sin(t) * K + (1 - torch.cos(t)) * K.mm(K)
    scale = 1 + (torch.rand(1) * 2 * c["delta"] - c["delta"]).expand(1, 3).to(dev)
    flip = not bool(torch.rand(1, device=dev) > c["flip_p"])
    for i in range(nag.num_levels):
        d = nag[i]
        d.pos = d.pos @ R.T
        d.normal = t_up(d.normal @ R.T)
        if d.edge_attr is not None:
            d.edge_attr[:, :3] = d.edge_attr[:, :3] @ R.T
    for i in range(nag.num_levels):
        d = nag[i]
        d.pos = d.pos * scale
        d.normal = torch.nn.functional.normalize(d.normal * scale, dim=1)
        if d.edge_attr is not None:
            d.edge_attr[:, :3] *= scale
            d.edge_attr[:, 3:] *= scale.norm()
    if flip:
        for i in range(nag.num_levels):
            d = nag[i]
            d.pos[:, 0] *= -1
            d.normal[:, 0] *= -1
            t_up(d.normal)
            if d.edge_attr is not None:
                d.edge_attr[:, :3][:, 0] *= -1


def t_features(nag, c):
    t_jitter(nag, POINT_KEYS, c["feat_jitter"], 2 * c["feat_jitter"])
    t_jitter(nag, ["edge_attr"], c["edge_jitter"], 2 * c["edge_jitter"])
    for i in range(nag.num_levels):
        for k in POINT_KEYS:
            t_dropout(nag[i][k], c["feat_drop"], 1)
        if nag[i].edge_attr is not None:
            t_dropout(nag[i].edge_attr, c["edge_drop"], 1)


def t_color(nag, c):
    t_jitter(nag, ["rgb"], c["rgb_jitter"], 2 * c["rgb_jitter"])
    for i in range(nag.num_levels):
        rgb = nag[i].rgb
        if torch.rand(1, device=rgb.device) < c["contrast"]:
            lo, hi = rgb.min(dim=0).values.view(1, -1), rgb.max(dim=0).values.view(1, -1)
            blend = torch.rand(1, device=rgb.device)
            nag[i].rgb = (1 - blend) * rgb + blend * ((rgb - lo) / (hi - lo))
    for i in range(nag.num_levels):
        if torch.rand(1, device=nag[i].rgb.device) < c["rgb_drop"]:
            nag[i].rgb *= 0


def stepwise(c):
    geo = [T.NAGJitterKey(key="pos", sigma=c["pos_jitter"], trunc=c["voxel"]),
           T.RandomTiltAndRotate(phi=c["phi"], theta=c["theta"]), T.RandomAnisotropicScale(delta=c["delta"]),
           T.RandomAxisFlip(p=c["flip_p"])]
    feat = [T.NAGJitterKey(key=POINT_KEYS, sigma=c["feat_jitter"], trunc=2 * c["feat_jitter"]),
            T.NAGJitterKey(key="edge_attr", sigma=c["edge_jitter"], trunc=2 * c["edge_jitter"]),
            T.NAGDropoutColumns(p=c["feat_drop"], key=POINT_KEYS, inplace=True),
            T.NAGDropoutColumns(p=c["edge_drop"], key="edge_attr", inplace=True),
            T.NAGDropoutRows(p=c["row_drop"], key=POINT_KEYS), T.NAGDropoutRows(p=c["row_drop"], key="edge_attr")]
    col = [T.NAGJitterKey(key="rgb", sigma=c["rgb_jitter"], trunc=2 * c["rgb_jitter"]),
           T.NAGColorAutoContrast(p=c["contrast"]), T.NAGColorDrop(p=c["rgb_drop"])]
    return geo, feat, col


def fused(c):
    geo = [T.GeometricAugmentation(pos_jitter=c["pos_jitter"], trunc=c["voxel"], phi=c["phi"], theta=c["theta"],
                                   delta=c["delta"], flip_axis=0, flip_p=c["flip_p"])]
    feat = [T.FeatureAugmentation(key=POINT_KEYS, sigma=c["feat_jitter"], trunc=2 * c["feat_jitter"],
                                  p_columns=c["feat_drop"], p_rows=c["row_drop"]),
            T.FeatureAugmentation(key="edge_attr", sigma=c["edge_jitter"], trunc=2 * c["edge_jitter"],
                                  p_columns=c["edge_drop"], p_rows=c["row_drop"])]
    col = [T.ColorAugmentation(sigma=c["rgb_jitter"], trunc=2 * c["rgb_jitter"], p_contrast=c["contrast"],
                               p_drop=c["rgb_drop"])]
    return geo, feat, col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene", nargs="?", default="T")
    ap.add_argument("--leg", default="all", choices=["all", "torch", "stepwise", "fused"])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nag7, nag18 = make_nag(a.scene, dev, 7), make_nag(a.scene, dev, 18)
    floats = sum(nag7[i][k].numel() for i in range(3) for k in ("pos", "normal", "edge_attr", "rgb")
                 if nag7[i].get(k) is not None)
    floats += sum(nag18[i][k].numel() for i in range(3) for k in POINT_KEYS + ["edge_attr"]
                  if nag18[i].get(k) is not None)
    print(f"scene {a.scene}: levels {[nag7[i].pos.shape[0] for i in range(3)]}, "
          f"{floats * 8 / 1e9:.4f} GB for one read and one write of every tensor touched")

    def chain(groups):
        geo, feat, col = groups

        def run():
            for t in geo:
                t(nag7)
            for t in feat:
                t(nag18)
            for t in col:
                t(nag7)
        return run

    def torch_leg():
        t_geometry(nag7, CFG)
        t_features(nag18, CFG)
        t_color(nag7, CFG)

    legs = [("torch", torch_leg), ("stepwise", chain(stepwise(CFG))), ("fused", chain(fused(CFG)))]
    for name, fn in legs:
        if a.leg not in ("all", name):
            continue
        torch.manual_seed(0)
        med, best, wall = timed(fn, a.reps)
        torch.manual_seed(0)
        before = dict(A.LAUNCHES)
        with Count() as cnt:
            fn()
        torch.cuda.synchronize()
        k, f = A.LAUNCHES["kernels"] - before["kernels"], A.LAUNCHES["fills"] - before["fills"]
        print(f"{name:9s} device {med:.3f} ms median / {best:.3f} ms min, host wall {wall:.3f} ms median over "
              f"{a.reps} calls (+ 2 warm-up); one call: {k} kernel launches of the package (+ {f} fills), "
              f"{cnt.ops} torch device operators, {cnt.reads} host reads; "
              f"{floats * 8 / med / 1e6:.0f} GB/s of the minimum traffic")


if __name__ == "__main__":
    main()
