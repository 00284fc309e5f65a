"""CPU suite of the augmentation block: the f64 restatement (tests/augment_reference.py) against
the fixture the reference's own classes produced (tests/golden/augment.npz), the transform
classes on CPU tensors driven with the fixture's recorded draws, the order in which ``draw``
consumes torch's CPU generator, fused == stepwise bit for bit, and the reference's quirks.

Exact: flips, sign fixes, drops, zeroed rows / columns, ``pos * scale``.  Bounded: rotation,
normalisation, contrast - by the reference's own f32 deviation from the f64 restatement
(``REFERENCE_DEVIATION``, measured and printed by ``test_reference_deviation``) for the
restatement, and by ``MARGIN`` times it for code whose operation order differs from torch's."""
import os

import numpy as np
import pytest
import torch

import augment_reference as AR
from superpoint_transformer_amd import augment as A
from superpoint_transformer_amd import transforms as T
from superpoint_transformer_amd.data import NAG, Data

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("pos", "normal", "rgb", "linearity", "edge_attr")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(HERE, "golden", "augment.npz")))
    return _cache["g"]


def nag_of(case, device="cpu", side="in"):
    g = golden()
    levels = []
    for i in range(3):
        d = Data()
        for k in KEYS:
            v = g.get(f"{case}/L{i}/{k}/{side}")
            if v is not None:
                d[k] = torch.from_numpy(v.copy()).to(device)
        levels.append(d)
    return NAG(levels)


def expected(case, i, k):
    return golden()[f"{case}/L{i}/{k}/out"]


def tensors(case):
    g = golden()
    return [(i, k) for i in range(3) for k in KEYS if f"{case}/L{i}/{k}/in" in g]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_case(case, nag, bounded, margin=AR.MARGIN, report=None):
    """Every tensor of ``nag`` against the fixture's output: keys of ``bounded`` (key ->
    REFERENCE_DEVIATION name) within margin x the recorded deviation, everything else bitwise."""
    for i, k in tensors(case):
        got = nag[i][k].detach().cpu().numpy()
        want = expected(case, i, k)
        if k in bounded:
            dev = AR.relative_deviation(got, want)
            if report is not None:
                report[(case, bounded[k])] = max(report.get((case, bounded[k]), 0.0), dev)
            assert dev <= margin * AR.REFERENCE_DEVIATION[bounded[k]], (case, i, k, dev)
        else:
            assert same_bits(got, want), (case, i, k)


# ---------------------------------------------------------------------------
def test_generator_restatements_agree():
    for seed in (0, 1, 12345678901234567, 2 ** 63 + 5, 2 ** 64 - 1):
        idx = np.array([0, 1, 2, 63, 64, 2 ** 31, 2 ** 32 + 7, 2 ** 40 + 1], dtype=np.uint64)
        want = [AR.rand32_scalar(seed, int(i)) for i in idx]
        assert AR.rand32(seed, idx).tolist() == want
        assert A.rand32(seed, torch.from_numpy(idx.astype(np.int64))).tolist() == want
    n = 10000
    u = A.unit(77, torch.arange(n)).numpy()
    assert u.dtype == np.float32 and np.array_equal(u.astype(np.float64), AR.decision_uniform(77, np.arange(n)))
    for p in (0.3, 0.5, 0.2):
        mine = (A.unit(77, torch.arange(n)) < torch.tensor(p, dtype=torch.float32)).numpy()
        assert np.array_equal(mine, AR.decisions(77, np.arange(n), p))


def measured_reference_deviation():
    """The reference's f32 outputs against the f64 restatement, per bounded map."""
    g = golden()
    dev = {k: 0.0 for k in AR.REFERENCE_DEVIATION}

    def upd(name, got, want):
        dev[name] = max(dev[name], AR.relative_deviation(got, want))

    R, s = g["tilt/R"], g["scale/scale"]
    for i in range(3):
        upd("rotate_pos", g[f"tilt/L{i}/pos/out"], AR.tilt_pos(g[f"tilt/L{i}/pos/in"], R))
        upd("rotate_normal", g[f"tilt/L{i}/normal/out"], AR.tilt_normal(g[f"tilt/L{i}/normal/in"], R))
        upd("scale_normal", g[f"scale/L{i}/normal/out"], AR.scale_normal(g[f"scale/L{i}/normal/in"], s))
        if i:
            upd("rotate_edge", g[f"tilt/L{i}/edge_attr/out"], AR.tilt_edge(g[f"tilt/L{i}/edge_attr/in"], R))
            upd("scale_edge", g[f"scale/L{i}/edge_attr/out"], AR.scale_edge(g[f"scale/L{i}/edge_attr/in"], s))
        for case in ("contrast", "contrast_fixed"):
            if g[f"{case}/taken/L{i}"]:
                b = float(g[f"{case}/blend/L{i}"])
                upd("contrast", g[f"{case}/L{i}/rgb/out"], AR.contrast(g[f"{case}/L{i}/rgb/in"], b))
    return dev


def test_reference_deviation():
    """The bounded maps: what the reference's f32 deviates from the f64 restatement, printed and
    held against the recorded ``REFERENCE_DEVIATION`` (profiles/r15a_augment_errors.txt)."""
    dev = measured_reference_deviation()
    for k, v in dev.items():
        print(f"reference f32 vs f64 restatement  {k:14s} {v:.4e}  (recorded {AR.REFERENCE_DEVIATION[k]:.4e})")
    for k, v in dev.items():
        assert 0.0 < v <= AR.REFERENCE_DEVIATION[k], (k, v)
        assert AR.REFERENCE_DEVIATION[k] < 1e-6, k          # f32 rounding, not a different map


def test_restatement_reproduces_fixture_exactly_where_exact():
    g = golden()
    s = g["scale/scale"]
    for i in range(3):
        # pos * scale: one f32 product
        assert same_bits(g[f"scale/L{i}/pos/out"], g[f"scale/L{i}/pos/in"] * s.astype(np.float32))
        for case, flip in (("flip_yes", True), ("flip_no", False)):
            assert bool(g[f"{case}/flip"]) == flip
            for k, fn in (("pos", AR.flip_pos), ("normal", AR.flip_normal), ("edge_attr", AR.flip_edge)):
                if f"{case}/L{i}/{k}/in" not in g:
                    continue
                a = g[f"{case}/L{i}/{k}/in"]
                want = fn(a, int(g[f"{case}/axis"])) if flip else a
                assert same_bits(g[f"{case}/L{i}/{k}/out"], want), (case, i, k)
        # nothing moves with phi = 0 although R is a real rotation
        for k in KEYS:
            if f"tilt_phi0/L{i}/{k}/in" in g:
                assert same_bits(g[f"tilt_phi0/L{i}/{k}/out"], g[f"tilt_phi0/L{i}/{k}/in"])
        # the sign fix of the rotated normals is exact in its DECISION
        rot = AR.rotate(g[f"tilt/L{i}/normal/in"], g["tilt/R"])
        sure = np.abs(rot[:, 2]) > 1e-5
        assert (g[f"tilt/L{i}/normal/out"][:, 2] >= 0).all()
        assert np.array_equal(np.sign(AR.upward(rot)[sure, 0]), np.sign(g[f"tilt/L{i}/normal/out"][sure, 0]))
        for case, fn, tag in (("dropcols", AR.drop_columns, "cols"), ("droprows", AR.drop_rows, "rows")):
            for k in ("linearity", "edge_attr"):
                if f"{case}/L{i}/{k}/in" in g:
                    want = fn(g[f"{case}/L{i}/{k}/in"], g[f"{case}/{tag}/L{i}/{k}"])
                    assert same_bits(g[f"{case}/L{i}/{k}/out"], want)
        if g[f"colordrop/taken/L{i}"]:
            assert same_bits(g[f"colordrop/L{i}/rgb/out"], AR.color_drop(g[f"colordrop/L{i}/rgb/in"]))
    assert (rot[:, 2] < 0).any()
    # the constant column: 0 / 0
    assert np.isnan(AR.contrast(g["contrast_fixed/L1/rgb/in"], 0.35)[:, 1]).all()
    # the reference's own jitter stays inside the truncation
    d = g["jitter/L0/pos/out"].astype(np.float64) - g["jitter/L0/pos/in"]
    assert np.abs(d).max() <= 0.03 + 1e-6 and 0.012 < d.std() < 0.02


def test_noise_formula_f32_deviation():
    """The noise formula evaluated with torch f32 CPU ops on the restatement's uniforms against
    f64, in units of sigma (indicative for the untruncated form: ill-conditioned at the tail)."""
    n = 1 << 20
    for (sigma, trunc), recorded in AR.NOISE_DEVIATION.items():
        u = AR.noise_uniform(3, np.arange(n))
        lo, hi = AR.noise_bounds(sigma, trunc)
        ref = AR.noise_from_uniform(u, sigma, trunc)
        t = torch.from_numpy(u).float()
        z = torch.erfinv(lo + t * (hi - lo)) * (sigma * np.sqrt(2.0))
        if trunc > 0:
            z = z.clamp(-trunc, trunc)
        ok = torch.isfinite(z).numpy()                       # f32 u rounds to 1 at the very top
        dev = np.abs(z.numpy().astype(np.float64)[ok] - ref[ok]).max() / sigma
        print(f"noise f32 formula vs f64  sigma {sigma} trunc {trunc}: {dev:.3e} sigma "
              f"(recorded {recorded:.3e}), non-finite in f32: {int((~ok).sum())}")
        assert dev <= 2.0 * recorded, (sigma, trunc, dev)
        assert np.isfinite(ref).all()
        if trunc > 0:
            assert np.abs(ref).max() <= trunc
        else:
            top = AR.noise_from_uniform(np.array([1 - 2.0 ** -25, 2.0 ** -25]), sigma, trunc)
            assert np.abs(ref).max() <= top[0] and top[0] == -top[1]
            assert 5.41 < top[0] / sigma < 5.43                # the tail ends at about 5.4 sigma
        ks = AR.ks_distance(ref, sigma, trunc)
        assert ks <= np.sqrt(np.log(2 / 1e-9) / (2 * n)), ks
        assert abs(AR.lag1(ref)) <= 6 / np.sqrt(n)


# ---------------------------------------------------------------------------
# the classes on CPU tensors, driven with the recorded draws
# ---------------------------------------------------------------------------
def test_classes_reproduce_fixture_cpu():
    run_classes_against_fixture("cpu")


def run_classes_against_fixture(device, report=None):
    g = golden()
    for case, phi in (("tilt", 60), ("tilt_phi0", 0)):
        nag = nag_of(case, device)
        t = T.RandomTiltAndRotate(phi=phi, theta=180)
        t.apply(nag, {"skip": phi == 0, "R": torch.from_numpy(g[f"{case}/R"])})
        check_case(case, nag, {} if phi == 0 else
                   {"pos": "rotate_pos", "normal": "rotate_normal", "edge_attr": "rotate_edge"},
                   report=report)
    nag = nag_of("scale", device)
    T.RandomAnisotropicScale(delta=0.2).apply(nag, {"scale": torch.from_numpy(g["scale/scale"])})
    check_case("scale", nag, {"normal": "scale_normal", "edge_attr": "scale_edge"}, report=report)
    for case in ("flip_yes", "flip_no"):
        nag = nag_of(case, device)
        T.RandomAxisFlip(axis=1, p=0.5).apply(nag, {"flip": bool(g[f"{case}/flip"]), "axis": 1})
        check_case(case, nag, {})
    nag = nag_of("dropcols", device)
    params = {(i, k): A.column_mask(g[f"dropcols/cols/L{i}/{k}"])
              for i in (1, 2) for k in ("linearity", "edge_attr")}
    T.NAGDropoutColumns(level="1+", p=0.3, key=["linearity", "edge_attr"], inplace=True).apply(nag, params)
    check_case("dropcols", nag, {})
    for case, blend in (("contrast", None), ("contrast_fixed", 0.35)):
        nag = nag_of(case, device)
        params = {}
        for i in range(3):
            if g[f"{case}/taken/L{i}"]:
                b = torch.tensor(g[f"{case}/blend/L{i}"])
                params[(i, "rgb")] = (float(b), float(1 - b)) if blend is None else (blend, 1.0 - blend)
        T.NAGColorAutoContrast(p=0.6, blend=blend).apply(nag, params)
        check_case(case, nag, {"rgb": "contrast"}, report=report)
        assert np.isnan(nag[1]["rgb"].cpu().numpy()[:, 1]).all() == bool(g[f"{case}/taken/L1"])
    nag = nag_of("colordrop", device)
    T.NAGColorDrop(p=0.5).apply(nag, {(i, "rgb"): True for i in range(3) if g[f"colordrop/taken/L{i}"]})
    check_case("colordrop", nag, {})
    assert np.signbit(nag[2]["rgb"].cpu().numpy()).any()


def test_row_dropout_and_jitter_follow_the_stream_cpu():
    run_stream_classes("cpu")


def run_stream_classes(device):
    """Row dropout and jitter have no recorded draw to replay (the reference draws them on the
    device generator): they follow the restated stream."""
    g = golden()
    nag = nag_of("droprows", device)
    params = {(i, "edge_attr"): (0.3, 1000 + i) for i in (1, 2)}
    T.NAGDropoutRows(level="all", p=0.3, key="edge_attr", inplace=True).apply(nag, params)
    for i in (1, 2):
        a = g[f"droprows/L{i}/edge_attr/in"]
        rows = AR.dropped_rows(1000 + i, a.shape[0], 0.3)
        assert same_bits(nag[i]["edge_attr"].cpu().numpy(), AR.drop_rows(a, rows))
    assert 15 <= AR.dropped_rows(1001, 120, 0.3).size <= 60
    nag = nag_of("jitter", device)
    T.NAGJitterKey(key="pos", sigma=0.03, trunc=0.03).apply(
        nag, {(i, "pos"): (0.03, 0.03, 50 + i) for i in range(3)})
    for i in range(3):
        a = g[f"jitter/L{i}/pos/in"]
        want = AR.jitter(a, 50 + i, 0.03, 0.03)
        got = nag[i]["pos"].cpu().numpy().astype(np.float64)
        # one f32 rounding of the sum (|pos| < 32: ulp 2e-6) plus the noise's own deviation
        assert np.abs(got - want).max() <= 2.0 ** -19 + AR.MARGIN * AR.NOISE_DEVIATION[(0.03, 0.03)] * 0.03
        assert np.abs(got - a).max() <= 0.03 + 2.0 ** -19


def test_new_tensor_unless_inplace():
    nag = nag_of("dropcols")
    before = nag[1]["edge_attr"]
    keep = before.clone()
    T.NAGDropoutColumns(level=1, p=0.3, key="edge_attr", inplace=False).apply(nag, {(1, "edge_attr"): 0b101})
    assert nag[1]["edge_attr"] is not before and torch.equal(before, keep)
    assert (nag[1]["edge_attr"][:, [0, 2]] == 0).all() and torch.equal(nag[1]["edge_attr"][:, 1], keep[:, 1])
    nag = nag_of("dropcols")
    before = nag[1]["edge_attr"]
    T.NAGDropoutColumns(level=1, p=0.3, key="edge_attr", inplace=True).apply(nag, {(1, "edge_attr"): 0b101})
    assert nag[1]["edge_attr"] is before and (before[:, 0] == 0).all()


def test_to_mean_composition():
    nag = nag_of("dropcols")
    a = nag[1]["edge_attr"].clone()
    T.NAGDropoutColumns(level=1, p=0.3, key="edge_attr", inplace=True, to_mean=True).apply(
        nag, {(1, "edge_attr"): 0b1000})
    want = a.clone()
    want[:, 3] = a.mean(dim=0)[3]
    assert torch.equal(nag[1]["edge_attr"], want)
    nag = nag_of("droprows")
    a = nag[1]["edge_attr"].clone()
    T.NAGDropoutRows(level=1, p=0.3, key="edge_attr", inplace=True, to_mean=True).apply(
        nag, {(1, "edge_attr"): (0.3, 9)})
    rows = torch.from_numpy(AR.dropped_rows(9, a.shape[0], 0.3))
    want = a.clone()
    want[rows] = a.mean(dim=0)
    assert torch.equal(nag[1]["edge_attr"], want)


# ---------------------------------------------------------------------------
# draw: torch's CPU generator in the documented order
# ---------------------------------------------------------------------------
def seeds_after(seed, n):
    torch.manual_seed(seed)
    return [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(n)]


def test_draw_order():
    g = golden()
    nag = nag_of("tilt")
    # tilt: the MultivariateNormal sample, then the angle; R as the reference's own R
    torch.manual_seed(int(g["tilt/seed"]))
    p = T.RandomTiltAndRotate(phi=60, theta=180).draw(nag)
    assert not p["skip"] and np.abs(p["R"].numpy() - g["tilt/R"]).max() <= 1e-6   # sin / cos: to an ulp
    after = torch.rand(1)
    torch.manual_seed(int(g["tilt/seed"]))
    torch.distributions.MultivariateNormal(torch.zeros(2), torch.eye(2)).sample()
    torch.rand(1)
    assert torch.equal(after, torch.rand(1))
    # phi = 0: only the angle is drawn, R is still a rotation, and it is skipped
    torch.manual_seed(int(g["tilt_phi0/seed"]))
    p = T.RandomTiltAndRotate(phi=0, theta=180).draw(nag)
    assert p["skip"] and np.abs(p["R"].numpy() - g["tilt_phi0/R"]).max() <= 1e-6
    after = torch.rand(1)
    torch.manual_seed(int(g["tilt_phi0/seed"]))
    torch.rand(1)
    assert torch.equal(after, torch.rand(1))
    # scale: one rand(1) shared by the three axes
    torch.manual_seed(int(g["scale/seed"]))
    p = T.RandomAnisotropicScale(delta=0.2).draw(nag)
    assert same_bits(p["scale"].numpy(), g["scale/scale"]) and len(set(p["scale"].tolist())) == 1
    torch.manual_seed(int(g["scale/seed"]))
    u = torch.rand(1)
    assert torch.equal(p["scale"], (1 + (u * 2 * 0.2 - 0.2)).expand(3))
    # flip
    for case in ("flip_yes", "flip_no"):
        torch.manual_seed(int(g[f"{case}/seed"]))
        assert T.RandomAxisFlip(axis=1, p=0.5).draw(nag)["flip"] == bool(g[f"{case}/flip"])
    # column dropout: the reference's own columns under the reference's seed
    nag = nag_of("dropcols")
    torch.manual_seed(int(g["dropcols/seed"]))
    p = T.NAGDropoutColumns(level="1+", p=0.3, key=["linearity", "edge_attr"], inplace=True).draw(nag)
    assert list(p) == [(1, "linearity"), (1, "edge_attr"), (2, "linearity"), (2, "edge_attr")]
    for (i, k), mask in p.items():
        assert mask == A.column_mask(g[f"dropcols/cols/L{i}/{k}"])
    # colours: the reference's own decisions and blends under the reference's seed
    for case, blend in (("contrast", None), ("contrast_fixed", 0.35)):
        nag = nag_of(case)
        torch.manual_seed(int(g[f"{case}/seed"]))
        p = T.NAGColorAutoContrast(p=0.6 if blend is None else 1.0, blend=blend).draw(nag)
        for i in range(3):
            assert ((i, "rgb") in p) == bool(g[f"{case}/taken/L{i}"])
            if (i, "rgb") in p:
                assert np.float32(p[(i, "rgb")][0]) == g[f"{case}/blend/L{i}"]
    nag = nag_of("colordrop")
    torch.manual_seed(int(g["colordrop/seed"]))
    p = T.NAGColorDrop(p=0.5).draw(nag)
    assert [(i, "rgb") in p for i in range(3)] == [bool(g[f"colordrop/taken/L{i}"]) for i in range(3)]
    # jitter and row dropout: one seed per (level, key) present, levels then keys
    nag = nag_of("droprows")
    torch.manual_seed(5)
    p = T.NAGJitterKey(key=["pos", "missing", "edge_attr"], sigma=[0.1, 0.0, 0.2], trunc=0.3).draw(nag)
    s = seeds_after(5, 3)
    assert p == {(0, "pos"): (0.1, 0.3, s[0]), (2, "pos"): (0.2, 0.3, s[1]),
                 (2, "edge_attr"): (0.2, 0.3, s[2])}
    torch.manual_seed(5)
    p = T.NAGDropoutRows(level="all", p=0.3, key=["linearity", "edge_attr"]).draw(nag)
    s = seeds_after(5, 5)
    assert list(p) == [(0, "linearity"), (1, "linearity"), (1, "edge_attr"), (2, "linearity"), (2, "edge_attr")]
    assert [v[1] for v in p.values()] == s and all(v[0] == 0.3 for v in p.values())


# ---------------------------------------------------------------------------
# fused == stepwise
# ---------------------------------------------------------------------------
def train_nag(device="cpu", edge_cols=7):
    nag = nag_of("dropcols" if edge_cols == 18 else "tilt", device)
    for i in range(3):
        nag[i]["mean_normal"] = nag[i]["normal"].flip(0).contiguous()
        nag[i]["hsv"] = nag[i]["rgb"].flip(1).contiguous()
    return nag


def fused_and_stepwise(device, seed=31):
    """[(name, fused nag, stepwise nag)] under the same torch.manual_seed."""
    out = []
    geo = dict(pos_jitter=0.03, trunc=0.03, phi=60, theta=180, delta=0.2, flip_axis=0, flip_p=1.0)
    a, b = train_nag(device), train_nag(device)
    torch.manual_seed(seed)
    T.GeometricAugmentation(**geo)(a)
    torch.manual_seed(seed)
    for t in (T.NAGJitterKey(key="pos", sigma=0.03, trunc=0.03), T.RandomTiltAndRotate(phi=60, theta=180),
              T.RandomAnisotropicScale(delta=0.2), T.RandomAxisFlip(axis=0, p=1.0)):
        t(b)
    out.append(("geometric", a, b))
    keys = ["linearity", "edge_attr"]
    a, b = train_nag(device, 18), train_nag(device, 18)
    torch.manual_seed(seed)
    T.FeatureAugmentation(key=keys, sigma=0.01, trunc=0.02, p_columns=0.3, p_rows=0.3)(a)
    torch.manual_seed(seed)
    for t in (T.NAGJitterKey(key=keys, sigma=0.01, trunc=0.02),
              T.NAGDropoutColumns(p=0.3, key=keys, inplace=True), T.NAGDropoutRows(p=0.3, key=keys)):
        t(b)
    out.append(("feature", a, b))
    a, b = train_nag(device), train_nag(device)
    torch.manual_seed(seed)
    T.ColorAugmentation(sigma=0.05, trunc=0.1, p_contrast=0.7, blend=None, p_drop=0.3)(a)
    torch.manual_seed(seed)
    for t in (T.NAGJitterKey(key="rgb", sigma=0.05, trunc=0.1), T.NAGColorAutoContrast(p=0.7),
              T.NAGColorDrop(p=0.3)):
        t(b)
    out.append(("color", a, b))
    return out


def assert_same_nags(a, b, what):
    for i in range(3):
        assert sorted(a[i].keys) == sorted(b[i].keys)
        for k in a[i].keys:
            assert same_bits(a[i][k].cpu().numpy(), b[i][k].cpu().numpy()), (what, i, k)


def test_fused_equals_stepwise_cpu():
    first = fused_and_stepwise("cpu")
    for name, a, b in first:
        assert_same_nags(a, b, name)
    # something happened, and the same seed repeats itself
    base = {"geometric": train_nag(), "feature": train_nag(edge_cols=18), "color": train_nag()}
    for (name, a, _), (_, a2, _) in zip(first, fused_and_stepwise("cpu")):
        assert_same_nags(a, a2, name)
        changed = [k for i in range(3) for k in a[i].keys
                   if not same_bits(a[i][k].numpy(), base[name][i][k].numpy())]
        assert changed, name


# ---------------------------------------------------------------------------
# quirks
# ---------------------------------------------------------------------------
def test_quirks():
    nag = nag_of("tilt")
    # phi = 0 skips whatever theta is
    before = nag_of("tilt")
    torch.manual_seed(0)
    T.RandomTiltAndRotate(phi=0, theta=180)(nag)
    assert_same_nags(nag, before, "phi=0")
    # the per-axis standard deviation of the axis offset is sqrt(sigma), not sigma
    torch.manual_seed(1)
    t = T.RandomTiltAndRotate(phi=60, theta=0)
    sigma = 60 / 180 * np.pi / 3
    offs = []
    for _ in range(400):
        R = t.draw(nag)["R"]          # theta = 0: R = identity, so read the axis from the draws
        offs.append(R)
    assert all(torch.allclose(R, torch.eye(3), atol=1e-6) for R in offs)
    torch.manual_seed(1)
    xy = torch.stack([torch.distributions.MultivariateNormal(torch.zeros(2), torch.eye(2) * sigma).sample()
                      for _ in range(2000)])
    assert abs(float(xy.std()) - np.sqrt(sigma)) < 0.05 and abs(float(xy.std()) - sigma) > 0.15
    # flips when the draw is <= p
    real = torch.rand
    try:
        torch.rand = lambda *a, **k: torch.tensor([0.25])
        assert T.RandomAxisFlip(axis=0, p=0.25).draw()["flip"] is True
        assert T.RandomAxisFlip(axis=0, p=0.2499).draw()["flip"] is False
    finally:
        torch.rand = real
    # a 7-column assertion
    bad = nag_of("dropcols")          # 18 columns
    for t, p in ((T.RandomTiltAndRotate(phi=60), None), (T.RandomAnisotropicScale(), None),
                 (T.RandomAxisFlip(p=1.0), None)):
        with pytest.raises(AssertionError, match="exactly 7"):
            t(bad)
    # column dropout: the first missing key ends the level; row dropout: per-key
    nag = nag_of("dropcols")
    p = T.NAGDropoutColumns(p=0.5, key=["linearity", "missing", "edge_attr"]).draw(nag)
    assert list(p) == [(0, "linearity"), (1, "linearity"), (2, "linearity")]
    p = T.NAGDropoutColumns(p=0.5, key=["missing", "linearity"]).draw(nag)
    assert p == {}
    assert T.NAGDropoutColumns(p=0.0, key="linearity").draw(nag) == {}
    p = T.NAGDropoutRows(p=0.5, key=["missing", "linearity"]).draw(nag)
    assert list(p) == [(0, "linearity"), (1, "linearity"), (2, "linearity")]
    # jitter: strict raises on a missing key, sigma <= 0 skips
    with pytest.raises(ValueError):
        T.NAGJitterKey(key="missing", strict=True).draw(nag)
    assert T.NAGJitterKey(key="pos", sigma=0).draw(nag) == {}
    # colours: every key draws its own decision and its own blend
    nag = train_nag()
    nag[0]["mean_rgb"] = nag[0]["rgb"].clone()
    torch.manual_seed(3)
    p = T.NAGColorAutoContrast(p=1.0, level=0).draw(nag)
    assert list(p) == [(0, "rgb"), (0, "mean_rgb")] and p[(0, "rgb")] != p[(0, "mean_rgb")]
    torch.manual_seed(3)
    draws = [float(torch.rand(1)) for _ in range(6)]
    assert np.float32(p[(0, "rgb")][0]) == np.float32(draws[1])
    assert np.float32(p[(0, "mean_rgb")][0]) == np.float32(draws[3])
    torch.manual_seed(4)
    p = T.NAGColorDrop(p=0.5).draw(nag)
    torch.manual_seed(4)
    names = [(i, k) for i in range(3) for k in ("rgb", "mean_rgb", "lab", "mean_lab", "hsv", "mean_hsv")
             if nag[i].get(k) is not None]
    assert list(p) == [n for n in names if bool(torch.rand(1) < 0.5)]
    # x_idx addresses a column block of x in place
    nag = train_nag()
    nag[0]["x"] = torch.cat((nag[0]["linearity"], nag[0]["rgb"], nag[0]["pos"]), dim=1)
    x = nag[0]["x"]
    keep = x.clone()
    T.NAGColorDrop(p=1.0, x_idx=1, level=0).apply(nag, {(0, ("x", 1)): True})
    assert nag[0]["x"] is x and (x[:, 1:4] == 0).all()
    assert torch.equal(x[:, :1], keep[:, :1]) and torch.equal(x[:, 4:], keep[:, 4:])
    assert torch.equal(nag[0]["rgb"], train_nag()[0]["rgb"])
