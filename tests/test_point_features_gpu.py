"""GPU suite of PointFeatures (csrc/point_feat.hip, superpoint_transformer_amd/features.py).

Against the reference's own output (tests/golden/point_features.npz, made by
tests/golden/make_golden_point_features.py from the reference's source):
  * EXACT (same IEEE f32 operations): ``rgb`` as floats, ``v``, ``density`` (inf and 0 rows
    included), the columns ``AddKeysTo`` builds, the fused ``partition_input`` against the two
    steps;
  * ``h``, ``s`` and the three ``lab`` columns: max |kernel - reference| <= 4 x the reference's own
    deviation from the f64 restatement (``R.REFERENCE_DEVIATION``, measured by
    tests/test_point_features_reference_cpu.py, relative to the column's largest magnitude).
    The kernel's figures are printed before the assert and recorded in
    profiles/r11a_point_features_errors.txt.
The values never depend on the route: 4-points-per-lane path or tail, aligned or unaligned base,
dense or strided output, uint8 or the same colours as floats."""
import numpy as np
import pytest
import torch

import point_features_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 63, 65, 257, 100_003)
_Z = None
_BIG = {}


def golden():
    global _Z
    if _Z is None:
        _Z = load_golden("point_features.npz")
    return _Z


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def big(kind, dev):
    """100 004 random colours (row 0 holds a value > 1 in both encodings) and their dense
    results, computed once."""
    if kind not in _BIG:
        from superpoint_transformer_amd import features
        gen = torch.Generator().manual_seed(99)
        rgb = torch.randint(0, 256, (SIZES[-1] + 1, 3), generator=gen, dtype=torch.uint8)
        rgb[0] = torch.tensor([200, 100, 50], dtype=torch.uint8)
        rgb[1] = torch.tensor([255, 0, 17], dtype=torch.uint8)
        rgb = rgb.to(dev)
        if kind == "f32":
            rgb = rgb.float()                       # [0, 255] floats: divided like the bytes
        _BIG[kind] = (rgb, features.point_colors(rgb))
    return _BIG[kind]


@pytest.mark.parametrize("name", list(R.COLOR_SETS))
def test_colours_against_the_reference(name, dev):
    from superpoint_transformer_amd import features
    z = golden()
    rgb = torch.from_numpy(z[f"{name}_in"]).to(dev)
    out = features.point_colors(rgb, ("rgb", "hsv", "lab"))
    assert set(out) == {"rgb", "hsv", "lab"}
    for key in R.COLOR_KEYS:
        assert out[key].dtype == torch.float32 and tuple(out[key].shape) == tuple(rgb.shape)
    want = {key: torch.from_numpy(z[f"{name}_{key}"]) for key in R.COLOR_KEYS}
    assert torch.equal(out["rgb"].cpu(), want["rgb"])
    assert torch.equal(out["hsv"][:, 2].cpu(), want["hsv"][:, 2])
    rgb01 = z[f"{name}_rgb"]
    allrgb = np.concatenate([z[f"{s}_rgb"] for s in R.COLOR_SETS])
    for key in ("hsv", "lab"):
        f64 = getattr(R, key)(rgb01)
        scale = np.abs(getattr(R, key)(allrgb)).max(0)
        got = out[key].cpu().numpy()
        vs_ref = np.abs(got.astype(np.float64) - want[key].numpy().astype(np.float64)).max(0) / scale
        vs_f64 = np.abs(got.astype(np.float64) - f64).max(0) / scale
        equal = (got.view(np.uint32) == want[key].numpy().view(np.uint32)).sum(0)
        bound = R.MARGIN * np.array(R.REFERENCE_DEVIATION[key])
        print(f"\n{name} {key}: kernel vs reference {vs_ref}, kernel vs f64 {vs_f64}, bound {bound}, "
              f"bitwise-equal elements per column {equal} of {got.shape[0]}")
        assert (vs_ref <= bound).all()


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_values_do_not_depend_on_the_route(kind, n, dev):
    """A prefix (4-per-lane groups + tail), the same rows from an unaligned base, and outputs
    written into columns 2..4 of a 9-wide table: bitwise the dense result of the whole table."""
    from superpoint_transformer_amd import features
    rgb, full = big(kind, dev)
    prefix = features.point_colors(rgb[:n])
    shifted = features.point_colors(rgb[1:n + 1])
    if kind == "u8":
        assert rgb[1:n + 1].data_ptr() % 4 != 0
    for key in R.COLOR_KEYS:
        assert same_bits(prefix[key], full[key][:n]), key
        # row 1 holds 255 / 255.0: the flag is set without row 0 as well
        assert same_bits(shifted[key], full[key][1:n + 1]), key
    for key in R.COLOR_KEYS:
        table = torch.full((n, 9), -7.0, device=dev)
        res = features.point_colors(rgb[:n], (key,), out={key: table[:, 2:5]})
        assert res[key].data_ptr() == table[:, 2:5].data_ptr()
        assert same_bits(table[:, 2:5], full[key][:n]), key
        assert bool((table[:, :2] == -7).all()) and bool((table[:, 5:] == -7).all())
    # all three keys into one table at once
    table = torch.full((n, 11), -7.0, device=dev)
    features.point_colors(rgb[:n], out={"lab": table[:, 1:4], "rgb": table[:, 4:7],
                                        "hsv": table[:, 8:11]})
    assert same_bits(table[:, 1:4], full["lab"][:n]) and same_bits(table[:, 4:7], full["rgb"][:n])
    assert same_bits(table[:, 8:11], full["hsv"][:n])
    assert bool((table[:, 0] == -7).all()) and bool((table[:, 7] == -7).all())


def test_uint8_and_the_same_colours_as_floats_agree(dev):
    from superpoint_transformer_amd import features
    rgb, full = big("u8", dev)
    _, full_f = big("f32", dev)
    # (an IEEE division: torch's device kernel multiplies by 1 / 255 for a Python-number divisor)
    unit = (rgb.cpu().float() / 255).to(dev)
    as_unit = features.point_colors(unit)                        # max <= 1: not divided again
    for key in R.COLOR_KEYS:
        assert same_bits(full[key], full_f[key]), key
        assert same_bits(full[key], as_unit[key]), key


def test_max_flag_branches(dev):
    from superpoint_transformer_amd import features
    gen = torch.Generator().manual_seed(5)
    img = torch.randint(0, 2, (1001, 3), generator=gen, dtype=torch.uint8)
    out = features.point_colors(img.to(dev))
    assert torch.equal(out["rgb"].cpu(), img.float())            # all <= 1: NOT divided
    want = R.colors(img.numpy())
    assert np.array_equal(out["hsv"][:, 2].cpu().numpy(), want["hsv"][:, 2].astype(np.float32))
    img2 = img.clone()
    img2[1000, 2] = 2                                            # one value above 1, in the tail
    out2 = features.point_colors(img2.to(dev))
    assert torch.equal(out2["rgb"].cpu(), img2.float() / 255)
    f = torch.rand(1001, 3, generator=gen)
    out3 = features.point_colors(f.to(dev), "rgb")
    assert list(out3) == ["rgb"] and torch.equal(out3["rgb"].cpu(), f)
    f[777, 1] = 1.5                                              # a float image with one value > 1
    out4 = features.point_colors(f.to(dev), ("rgb",))
    assert torch.equal(out4["rgb"].cpu(), (f / 255).clamp(0, 1))
    f[3, 0] = -0.25                                              # clamped below as well
    f[777, 1] = 0.5
    out5 = features.point_colors(f.to(dev), ("rgb",))
    assert torch.equal(out5["rgb"].cpu(), f.clamp(0, 1))
    # other integer dtypes are cast like rgb.float()
    out6 = features.point_colors(img2.to(dev).long(), ("rgb",))
    assert same_bits(out6["rgb"], out2["rgb"])


def test_density_against_the_reference(dev):
    from superpoint_transformer_amd import features
    z = golden()
    idx13 = torch.from_numpy(z["knn_index13"]).to(dev)
    dist13 = torch.from_numpy(z["knn_distance13"]).to(dev)
    want = torch.from_numpy(z["density"])
    sliced = features.point_density(idx13[:, 1:], dist13[:, 1:])
    dense = features.point_density(idx13[:, 1:].contiguous(), dist13[:, 1:].contiguous())
    assert sliced.dtype == torch.float32 and tuple(sliced.shape) == (2000, 1)
    assert same_bits(sliced.cpu(), want) and same_bits(dense.cpu(), want)
    assert int(torch.isinf(sliced).sum()) == 2 and int((sliced == 0).sum()) == 100


@pytest.mark.parametrize("n", [1, 63, 65, 100_003])
@pytest.mark.parametrize("k", [1, 12, 45, 64, 255])
def test_density_shapes_contiguous_and_sliced(k, n, dev):
    from superpoint_transformer_amd import features
    gen = torch.Generator(device=dev).manual_seed(1000 * k + n % 997)
    idx = torch.randint(0, max(n, 2), (n, k + 1), generator=gen, device=dev)
    dist = torch.rand(n, k + 1, generator=gen, device=dev) + 0.01
    valid = torch.randint(0, k + 1, (n, 1), generator=gen, device=dev)
    valid[::3] = k                                               # full rows
    pad = torch.arange(k, device=dev).view(1, k) >= valid
    idx[:, 1:][pad] = -1
    dist[:, 1:][pad] = -1.0
    if n > 40:
        dist[40, 1:] = 0.0                                       # max 0: inf (0 / 0 = NaN if empty)
        idx[40, 1:] = 7
    want = torch.from_numpy(R.density(idx[:, 1:].cpu().numpy(), dist[:, 1:].cpu().numpy()))
    sliced = features.point_density(idx[:, 1:], dist[:, 1:])
    dense = features.point_density(idx[:, 1:].contiguous(), dist[:, 1:].contiguous())
    assert same_bits(sliced.cpu(), want)
    assert same_bits(dense.cpu(), want)
    if n > 40:
        assert bool(torch.isinf(sliced[40]))


def _cloud(dev, with_hsv=False):
    """20 000-point voxel-lattice cloud with the library's kNN (k = 12), colours, elevation."""
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.neighbors import knn_1
    from superpoint_transformer_amd.synthetic import make_voxel_cloud
    pos = make_voxel_cloud(20_000, voxel=0.03, seed=11, device=dev).contiguous()
    n = pos.shape[0]
    gen = torch.Generator(device=dev).manual_seed(3)
    nn, dist = knn_1(pos, 12, r_max=0.5)
    d = Data(pos=pos, neighbor_index=nn, neighbor_distance=dist,
             rgb=torch.randint(0, 256, (n, 3), generator=gen, device=dev, dtype=torch.uint8),
             elevation=torch.rand(n, 1, generator=gen, device=dev))
    if with_hsv:
        d.hsv = torch.full((n, 3), 0.25, device=dev)
    return d


def test_point_features_transform(dev):
    from superpoint_transformer_amd import features, transforms
    from superpoint_transformer_amd.neighbors import geometric_features
    data = _cloud(dev)
    n = data.num_nodes
    raw = data.rgb.clone()
    out = transforms.PointFeatures()(data)                       # keys=None: all of POINT_FEATURES
    assert out is data
    for key in features.GEOMETRIC_FEATURES + ["rgb", "hsv", "lab", "density"]:
        width = 3 if key in ("rgb", "hsv", "lab", "normal") else 1
        assert data[key].dtype == torch.float32 and tuple(data[key].shape) == (n, width), key
    assert "pos_room" not in data and "intensity" not in data
    table = geometric_features(data.pos, data.neighbor_index, k_min=5)
    for key, (lo, hi) in features.GEOF_SLICES.items():
        assert same_bits(data[key], table[:, lo:hi]), key
    colours = features.point_colors(raw)
    for key in R.COLOR_KEYS:
        assert same_bits(data[key], colours[key])
    assert same_bits(data.density, features.point_density(data.neighbor_index,
                                                          data.neighbor_distance))
    want = R.density(data.neighbor_index.cpu().numpy(), data.neighbor_distance.cpu().numpy())
    assert same_bits(data.density.cpu(), torch.from_numpy(want))


def test_overwrite_false_keeps_existing_keys_but_normalises_rgb(dev):
    from superpoint_transformer_amd import transforms
    data = _cloud(dev, with_hsv=True)
    raw = data.rgb.clone()
    kept = data.hsv
    transforms.PointFeatures(keys=["rgb", "hsv", "lab", "linearity"], overwrite=False)(data)
    assert data.hsv is kept and bool((data.hsv == 0.25).all())
    assert data.rgb.dtype == torch.float32 and torch.equal(data.rgb.cpu(), raw.cpu().float() / 255)
    assert "lab" in data and "linearity" in data and "density" not in data
    # rgb is normalised even when it is the only thing left to do, and twice is once
    before = data.rgb.clone()
    transforms.PointFeatures(keys=["rgb"], overwrite=False)(data)
    assert torch.equal(data.rgb, before)
    # without colours the colour keys are skipped
    data.rgb = None
    data.lab = None
    transforms.PointFeatures(keys=["lab", "density"])(data)
    assert "lab" not in data and "density" in data


PARTITION_CASES = {
    # S3DIS-like: rgb in both lists
    "s3dis": (["rgb", "linearity", "planarity", "scattering", "verticality", "elevation",
               "density", "normal"],
              ["rgb", "linearity", "planarity", "scattering", "verticality", "elevation"], False),
    # KITTI-360-like: hsv; a key of x that PointFeatures does not compute; density outside x
    "kitti360": (["hsv", "linearity", "planarity", "scattering", "verticality", "density"],
                 ["hsv", "elevation", "linearity", "planarity", "scattering", "verticality"], False),
    "all_colours_existing_x": (["rgb", "hsv", "lab", "normal", "curvature"],
                               ["lab", "normal", "rgb", "curvature", "hsv"], True),
}


@pytest.mark.parametrize("case", list(PARTITION_CASES))
def test_partition_input_equals_the_two_steps(case, dev):
    from superpoint_transformer_amd import features, transforms
    point_keys, partition_keys, with_x = PARTITION_CASES[case]
    a, b = _cloud(dev), _cloud(dev)
    if with_x:
        a.x = torch.arange(a.num_nodes * 2, device=dev, dtype=torch.float32).view(-1, 2)
        b.x = a.x.clone()
    transforms.PointFeatures(keys=point_keys)(a)
    transforms.AddKeysTo(keys=partition_keys, to="x", delete_after=False)(a)
    features.partition_input(b, point_keys, partition_keys)
    assert same_bits(a.x, b.x)
    assert sorted(a.keys) == sorted(b.keys)
    for key in a.keys:
        if torch.is_tensor(a[key]) and a[key].is_floating_point():
            assert same_bits(a[key], b[key]), key
    # the keys of x are views of its columns: one table, no second copy
    x = b.x
    lo, hi = x.data_ptr(), x.data_ptr() + x.numel() * 4
    for key in partition_keys:
        if key != "elevation":
            assert lo <= b[key].data_ptr() < hi, key
    # AddKeysTo's columns against the attributes themselves
    col = 2 if with_x else 0
    for key in partition_keys:
        w = a[key].shape[1]
        assert same_bits(a.x[:, col:col + w], a[key]), key
        col += w
    assert col == a.x.shape[1]


def test_partition_input_overwrite_false_and_missing_key(dev):
    from superpoint_transformer_amd import features, transforms
    a, b = _cloud(dev, with_hsv=True), _cloud(dev, with_hsv=True)
    keys = ["rgb", "hsv", "planarity"]
    transforms.PointFeatures(keys=keys, overwrite=False)(a)
    transforms.AddKeysTo(keys=["hsv", "planarity", "rgb"], delete_after=False)(a)
    features.partition_input(b, keys, ["hsv", "planarity", "rgb"], overwrite=False)
    assert same_bits(a.x, b.x) and bool((b.x[:, :3] == 0.25).all())
    with pytest.raises(Exception, match="should contain the attribute 'nope'"):
        features.partition_input(_cloud(dev), ["rgb"], ["rgb", "nope"])
    c = features.partition_input(_cloud(dev), ["rgb"], ["rgb", "nope"], strict=False)
    assert tuple(c.x.shape) == (c.num_nodes, 3)


def test_run_to_run_bitwise_reproducibility(dev):
    from superpoint_transformer_amd import features
    rgb, _ = big("u8", dev)
    z = golden()
    idx = torch.from_numpy(z["knn_index13"]).to(dev)[:, 1:]
    dist = torch.from_numpy(z["knn_distance13"]).to(dev)[:, 1:]

    def run():
        c = features.point_colors(rgb)
        cf = features.point_colors(rgb.float(), ("lab", "hsv"))
        d = features.point_density(idx, dist)
        p = features.partition_input(_cloud(dev), ["rgb", "lab", "density", "normal"],
                                     ["lab", "density", "normal", "elevation"])
        return [c["rgb"], c["hsv"], c["lab"], cf["hsv"], cf["lab"], d, p.x]

    first = [t.clone() for t in run()]
    for _ in range(2):
        for a, b in zip(first, run()):
            assert same_bits(a, b)


def test_argument_errors(dev):
    from superpoint_transformer_amd import features
    rgb = torch.zeros(8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="unknown colour keys"):
        features.point_colors(rgb, ("rgb", "xyz"))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        features.point_colors(torch.zeros(8, 4, device=dev))
    with pytest.raises(ValueError, match="adjacent"):
        features.point_colors(rgb, ("hsv",), out={"hsv": torch.zeros(3, 8, device=dev).t()})
    with pytest.raises(ValueError, match="float32 device tensor"):
        features.point_colors(rgb, ("hsv",), out={"hsv": torch.zeros(8, 3, device=dev).double()})
    with pytest.raises(ValueError, match="1..255"):
        features.point_density(torch.zeros(4, 256, dtype=torch.long, device=dev),
                               torch.zeros(4, 256, device=dev))
    with pytest.raises(ValueError, match="differ in shape"):
        features.point_density(torch.zeros(4, 5, dtype=torch.long, device=dev),
                               torch.zeros(4, 6, device=dev))
    empty = features.point_colors(rgb[:0])
    assert all(tuple(v.shape) == (0, 3) for v in empty.values())
    assert tuple(features.point_density(torch.zeros(0, 5, dtype=torch.long, device=dev),
                                        torch.zeros(0, 5, device=dev)).shape) == (0, 1)
