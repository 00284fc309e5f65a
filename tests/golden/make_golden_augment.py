"""Golden fixture for the augmentation block of the training chain, produced by the REFERENCE'S
OWN classes on the CPU: ``RandomTiltAndRotate``, ``RandomAnisotropicScale``, ``RandomAxisFlip``
(src/transforms/geometry.py), ``NAGJitterKey``, ``NAGDropoutColumns``, ``NAGDropoutRows`` with
their per-level classes and ``dropout`` (src/transforms/data.py, src/utils/dropout.py),
``NAGColorAutoContrast``, ``NAGColorDrop`` with their parents (src/transforms/point.py),
``rodrigues_rotation_matrix`` (src/utils/geometry.py), ``fill_list_with_string_indexing``
(src/utils/list.py) and ``NAG.apply_data_transform`` (src/data/nag.py), each cut out of its file
with ``ast``, unmodified.  Only inputs, outputs and the scalars the reference drew are stored
(tests/golden/augment.npz).

The NAG: three levels of 300 / 40 / 8 nodes with ``pos``, ``normal`` (unit, z >= 0), ``rgb``
(level 1: a CONSTANT green column; level 2: some NEGATIVE values), a 1-column ``linearity``,
and, at levels 1 and 2, ``edge_attr`` with 7 columns (geometry cases) or 18 (dropout cases).

Cases (``<case>/L<level>/<key>/in`` and ``/out``; scalars under ``<case>/...``):
  tilt         phi 60, theta 180 (normals change the sign of z: asserted)      R
  tilt_phi0    phi 0, theta 180: nothing moves                                 R
  scale        delta 0.2                                                       scale
  flip_yes / flip_no    axis 1, p 0.5, two seeds (asserted: one flips, one does not)   flip
  jitter       key pos, sigma 0.03, trunc 0.03 (the reference's own trunc_normal_)
  dropcols     level '1+', p 0.3, keys linearity + edge_attr (18)              cols/<level>/<key>
  droprows     level 'all', p 0.3, key edge_attr (18)                          rows/<level>/<key>
  contrast     p 0.6, blend None: per tensor 'taken', 'blend' (replayed from the seed: asserted)
  contrast_fixed  p 1.0, blend 0.35: the constant column gives NaN
  colordrop    p 0.5: per tensor 'taken'; negative inputs give -0

Usage (build container only): python tests/golden/make_golden_augment.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import augment_reference as AR  # noqa: E402

REF = mg.REF


def cut(path, names, ns, inside=None):
    """exec the definitions ``names`` of a reference file (top level, or methods of the class
    ``inside``), unmodified, in ``ns``."""
    tree = ast.parse(open(os.path.join(REF, path)).read())
    body = tree.body
    if inside:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == inside).body
    body = [n for n in body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), os.path.basename(path), "exec"), ns)


class DuckData:
    """What the transforms touch of a Data: attributes that read as None when absent."""

    def __init__(self, **attrs):
        self.__dict__.update(attrs)

    def __getattr__(self, key):
        if key.startswith("__"):
            raise AttributeError(key)
        return None

    def __getitem__(self, key):
        return self.__dict__[key]

    def __setitem__(self, key, value):
        self.__dict__[key] = value


def load_reference():
    ns = {"torch": torch, "np": np, "Transform": object}
    cut("src/utils/list.py", ["fill_list_with_string_indexing"], ns)
    cut("src/utils/dropout.py", ["dropout"], ns)
    cut("src/utils/geometry.py", ["cross_product_matrix", "rodrigues_rotation_matrix"], ns)
    ns["drawn_R"] = []
    rodrigues = ns["rodrigues_rotation_matrix"]

    def recording(axis, theta):
        R = rodrigues(axis, theta)
        ns["drawn_R"].append(R.clone())
        return R
    ns["rodrigues_rotation_matrix"] = recording

    class DuckNAG:
        def __init__(self, levels):
            self._list = levels
        device = torch.device("cpu")
        num_levels = property(lambda self: len(self._list))
        absolute_num_levels = num_levels
        start_i_level = 0
        end_i_level = property(lambda self: len(self._list) - 1)
        level_range = property(lambda self: range(len(self._list)))

        def __getitem__(self, i):
            return self._list[i]

        def assert_level_in_nag(self, i):
            assert 0 <= i < len(self._list)

    fns = {}
    cut("src/data/nag.py", ["apply_data_transform"], fns, inside="NAG")
    DuckNAG.apply_data_transform = fns["apply_data_transform"]
    ns["NAG"] = DuckNAG
    cut("src/transforms/geometry.py",
        ["RandomTiltAndRotate", "RandomAnisotropicScale", "RandomAxisFlip"], ns)
    cut("src/transforms/data.py",
        ["DropoutColumns", "NAGDropoutColumns", "DropoutRows", "NAGDropoutRows", "NAGJitterKey"], ns)
    cut("src/transforms/point.py",
        ["ColorTransform", "ColorAutoContrast", "NAGColorAutoContrast", "ColorDrop",
         "NAGColorDrop"], ns)
    # the per-level classes are called like Transform.__call__ does: through _process
    for name in ("DropoutColumns", "DropoutRows", "ColorAutoContrast", "ColorDrop"):
        ns[name].__call__ = lambda self, data: self._process(data)
    return ns


def make_levels(rng, edge_cols):
    levels = []
    for i, (n, e) in enumerate(((300, 0), (40, 120), (8, 20))):
        f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
        nrm = f(n, 3)
        nrm[:, 2] = np.abs(nrm[:, 2])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        rgb = rng.random((n, 3)).astype(np.float32)
        if i == 1:
            rgb[:, 1] = 0.5
        if i == 2:
            rgb[::2] -= 0.75
        d = dict(pos=f(n, 3) * np.float32(4.0), normal=nrm.astype(np.float32), rgb=rgb,
                 linearity=rng.random((n, 1)).astype(np.float32) + np.float32(0.1))
        if e:
            d["edge_attr"] = f(e, edge_cols)
        levels.append(d)
    return levels


def main():
    ns = load_reference()
    NAG = ns["NAG"]
    rng = np.random.default_rng(20250915)
    base = {7: make_levels(rng, 7), 18: make_levels(rng, 18)}
    out = {}

    def run(case, transform, seed, edge_cols=7):
        levels = [DuckData(**{k: torch.from_numpy(v.copy()) for k, v in lv.items()})
                  for lv in base[edge_cols]]
        nag = NAG(levels)
        torch.manual_seed(seed)
        transform._process(nag)
        for i, lv in enumerate(base[edge_cols]):
            for k, v in lv.items():
                got = nag[i][k]
                assert got.dtype == torch.float32 and tuple(got.shape) == v.shape, (case, i, k)
                out[f"{case}/L{i}/{k}/in"] = v
                out[f"{case}/L{i}/{k}/out"] = got.numpy().copy()
        out[f"{case}/seed"] = np.int64(seed)
        return nag

    def changed(case, i, k):
        a, b = out[f"{case}/L{i}/{k}/in"], out[f"{case}/L{i}/{k}/out"]
        return not np.array_equal(a, b, equal_nan=True)

    # ---- geometry ----
    for seed in range(3, 64):      # the first seed whose tilt sends a good share of normals down
        run("tilt", ns["RandomTiltAndRotate"](phi=60, theta=180), seed)
        out["tilt/R"] = ns["drawn_R"][-1].numpy()
        rot = AR.rotate(out["tilt/L0/normal/in"], out["tilt/R"])
        if (rot[:, 2] < 0).sum() > 10 and (rot[:, 2] > 0).sum() > 10:
            break
    else:
        raise AssertionError("no sign change of z")
    run("tilt_phi0", ns["RandomTiltAndRotate"](phi=0, theta=180), 4)
    out["tilt_phi0/R"] = ns["drawn_R"][-1].numpy()
    assert not any(changed("tilt_phi0", i, k) for i in range(3) for k in base[7][i])
    assert np.abs(out["tilt_phi0/R"] - np.eye(3)).max() > 0.1    # a real rotation, never applied

    run("scale", ns["RandomAnisotropicScale"](delta=0.2), 5)
    torch.manual_seed(5)
    delta = torch.tensor([0.2] * 3).abs().view(1, -1)
    scale = (1 + (torch.rand(1) * 2 * delta - delta)).view(3)
    out["scale/scale"] = scale.numpy()
    assert np.array_equal(out["scale/L0/pos/out"], out["scale/L0/pos/in"] * out["scale/scale"])

    seeds = {}
    for seed in range(100):
        torch.manual_seed(seed)
        seeds.setdefault(bool(torch.rand(1) <= 0.5), seed)
    for name, taken in (("flip_yes", True), ("flip_no", False)):
        run(name, ns["RandomAxisFlip"](axis=1, p=0.5), seeds[taken])
        out[f"{name}/flip"] = np.bool_(taken)
        out[f"{name}/axis"] = np.int64(1)
        assert changed(name, 0, "pos") == taken

    run("jitter", ns["NAGJitterKey"](key="pos", sigma=0.03, trunc=0.03), 6)

    # ---- dropouts (18-column edge_attr) ----
    run("dropcols", ns["NAGDropoutColumns"](level="1+", p=0.3, key=["linearity", "edge_attr"],
                                            inplace=True), 11, edge_cols=18)
    run("droprows", ns["NAGDropoutRows"](level="all", p=0.3, key="edge_attr"), 12, edge_cols=18)
    for case, axis, tag in (("dropcols", 0, "cols"), ("droprows", 1, "rows")):
        for i in range(3):
            for k in ("linearity", "edge_attr"):
                if f"{case}/L{i}/{k}/in" not in out:
                    continue
                a, b = out[f"{case}/L{i}/{k}/in"], out[f"{case}/L{i}/{k}/out"]
                assert (a != 0).all()
                idx = np.nonzero((b == 0).all(axis=axis))[0]
                out[f"{case}/{tag}/L{i}/{k}"] = idx.astype(np.int64)
                ref = AR.drop_columns(a, idx) if tag == "cols" else AR.drop_rows(a, idx)
                assert np.array_equal(ref, b), (case, i, k)
    assert out["dropcols/cols/L0/linearity"].size == 0
    assert out["dropcols/cols/L1/edge_attr"].size > 0 and out["droprows/rows/L1/edge_attr"].size > 0
    assert not changed("droprows", 0, "linearity")

    # ---- colours ----
    def replay_contrast(seed, p, blend):
        """The draws of NAGColorAutoContrast in its own order: per level, rgb only."""
        torch.manual_seed(seed)
        drawn = []
        for _ in range(3):
            taken = bool(torch.rand(1) < p)
            b = None
            if taken:
                b = torch.rand(1) if blend is None else blend
            drawn.append((taken, b))
        return drawn

    for case, p, blend, seed in (("contrast", 0.6, None, 21), ("contrast_fixed", 1.0, 0.35, 22)):
        if blend is None:          # a seed with both outcomes
            seed = next(s for s in range(200)
                        if len({t for t, _ in replay_contrast(s, p, blend)}) == 2)
        run(case, ns["NAGColorAutoContrast"](p=p, blend=blend), seed)
        for i, (taken, b) in enumerate(replay_contrast(seed, p, blend)):
            assert changed(case, i, "rgb") == taken, (case, i)
            out[f"{case}/taken/L{i}"] = np.bool_(taken)
            out[f"{case}/blend/L{i}"] = np.float32(float(b) if taken else 0.0)
            if taken:                # the reference's own expression reproduces its output
                rgb = torch.from_numpy(out[f"{case}/L{i}/rgb/in"])
                lo, hi = rgb.min(dim=0).values.view(1, -1), rgb.max(dim=0).values.view(1, -1)
                again = (1 - b) * rgb + b * ((rgb - lo) / (hi - lo))
                assert np.array_equal(again.numpy(), out[f"{case}/L{i}/rgb/out"], equal_nan=True)
    assert np.isnan(out["contrast_fixed/L1/rgb/out"][:, 1]).all()
    assert not np.isnan(out["contrast_fixed/L1/rgb/out"][:, 0]).any()

    seed = next(s for s in range(200) if len(set(
        (torch.manual_seed(s), [bool(torch.rand(1) < 0.5) for _ in range(3)])[1][1:])) == 2
        and (torch.manual_seed(s), [bool(torch.rand(1) < 0.5) for _ in range(3)])[1][2])
    run("colordrop", ns["NAGColorDrop"](p=0.5), seed)
    for i in range(3):
        b = out[f"colordrop/L{i}/rgb/out"]
        out[f"colordrop/taken/L{i}"] = np.bool_(changed("colordrop", i, "rgb"))
        if out[f"colordrop/taken/L{i}"]:
            assert (b == 0).all()
    assert out["colordrop/taken/L2"] and np.signbit(out["colordrop/L2/rgb/out"]).any()

    mg.save("augment.npz", **out)
    size = os.path.getsize(os.path.join(HERE, "augment.npz"))
    assert size < 900 * 1024, size
    print("augment.npz:", size, "bytes")


if __name__ == "__main__":
    main()
