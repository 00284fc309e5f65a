"""numpy restatement of the colour keys and the density of ``PointFeatures``
(src/transforms/point.py:116-182, src/utils/color.py:17-22, src/utils/features.py:8-86), shared
by tests/golden/make_golden_point_features.py and the point-feature tests.

``to_float_rgb`` and ``density`` are f32, operation by operation as the reference's (they are
compared bitwise).  ``hsv`` and ``lab`` are f64 on the f32 colours: the yardstick the f32 results
of the reference and of the kernel are measured against; ``lab`` rounds to 4 decimals where the
reference rounds.  Nothing here is imported from the reference."""
import numpy as np

COLOR_KEYS = ("rgb", "hsv", "lab")
# the colour sets of the fixture: name -> dtype of the stored input
COLOR_SETS = {"u8": np.uint8, "u8_small": np.uint8, "f32": np.float32, "f32_gt1": np.float32}

# max |reference f32 - f64 restatement| / max |f64| per output column over all 16 576 colour rows
# of tests/golden/point_features.npz (hsv: h / 360, s, v; lab: L, a, b, each / 100), measured by
# tests/test_point_features_reference_cpu.py and recorded in
# profiles/r11a_point_features_errors.txt.  The GPU suite allows the kernel MARGIN times this
# against the reference's output (the project's standing margin for an f32 kernel whose
# operation order may differ from torch's).
REFERENCE_DEVIATION = {"hsv": (8.1722e-08, 8.1897e-08, 0.0),
                       "lab": (8.9982e-06, 3.9698e-05, 1.4834e-05)}
MARGIN = 4.0

# Data.add_keys_to scenarios of the fixture.  Attributes of the 7-node Data: a [7, 1], b [7]
# (1-D), c [7, 3], x0 [7, 2] (stored as 'x' when with_x), short [5, 1] (wrong row count).
ADD_KEYS_CASES = {
    "order": dict(keys=["c", "a", "b"], to="x", strict=True, delete_after=False, with_x=False),
    "existing_x": dict(keys=["b", "c"], to="x", strict=True, delete_after=False, with_x=True),
    "delete_after": dict(keys=["a", "c"], to="x", strict=True, delete_after=True, with_x=True),
    "not_strict": dict(keys=["a", "missing", "b"], to="x", strict=False, delete_after=False,
                       with_x=False),
    "other_target": dict(keys=["a", "b"], to="feat", strict=True, delete_after=True, with_x=True),
    "single_string_key": dict(keys=["c"], to="x", strict=True, delete_after=False, with_x=False),
}
ADD_KEYS_ERRORS = {
    "missing_strict": dict(keys=["a", "missing"], to="x", strict=True, delete_after=False,
                           with_x=False),
    "row_mismatch": dict(keys=["a", "short"], to="x", strict=True, delete_after=False, with_x=True),
}


def add_keys_inputs():
    rng = np.random.default_rng(77)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return {"a": f(7, 1), "b": f(7), "c": f(7, 3), "x0": f(7, 2), "short": f(5, 1)}


def to_float_rgb(rgb):
    """f32 [N, 3]: / 255 when the global max is > 1, clamped to [0, 1]."""
    x = np.asarray(rgb).astype(np.float32)
    if x.size and x.max() > 1:
        x = x / np.float32(255)
    return np.clip(x, np.float32(0), np.float32(1))


def hsv(rgb01):
    """f64 [N, 3] (h / 360, s, v) of f32 colours in [0, 1]; first minimal channel on ties."""
    c = np.asarray(rgb01, dtype=np.float64)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    mx, mn = c.max(1), c.min(1)
    arg = c.argmin(1)                                   # first occurrence
    mm = mx - mn + 1e-10
    h1 = 60.0 * (g - r) / mm + 60.0
    h2 = 60.0 * (b - g) / mm + 180.0
    h3 = 60.0 * (r - b) / mm + 300.0
    h = np.choose(arg, (h2, h3, h1))
    return np.stack((h / 360.0, mm / (mx + 1e-10), mx), axis=1)


def round4(x):
    return np.rint(x * 1e4) / 1e4


M_XYZ = np.array([[0.4124, 0.2126, 0.0193], [0.3576, 0.7152, 0.1192], [0.1805, 0.0722, 0.9505]])
WHITE = np.array([95.047, 100.0, 108.883])
M_LAB = np.array([[0.0, 500.0, 0.0], [116.0, -500.0, 200.0], [0.0, 0.0, -200.0]])


def xyz_over_white(rgb01):
    c = np.asarray(rgb01, dtype=np.float64)
    lin = np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92) * 100.0
    return round4(lin @ M_XYZ) / WHITE


def lab(rgb01):
    """f64 [N, 3] lab / 100 of f32 colours in [0, 1]."""
    t = xyz_over_white(rgb01)
    f = np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 1 / 7.25)
    out = f @ M_LAB
    out[:, 0] -= 16.0
    return round4(out) / 100.0


def colors(rgb):
    """{'rgb': f32 (exact), 'hsv': f64, 'lab': f64} of a uint8 or float colour table."""
    c = to_float_rgb(rgb)
    return {"rgb": c, "hsv": hsv(c), "lab": lab(c)}


def density(neighbor_index, neighbor_distance):
    """f32 [N, 1], the reference's f32 operations: float(k) / (dmax * dmax)."""
    d = np.asarray(neighbor_distance, dtype=np.float32)
    k = (np.asarray(neighbor_index) >= 0).sum(1).astype(np.float32)
    dmax = d.max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (k / (dmax * dmax)).astype(np.float32).reshape(-1, 1)


def relative_deviation(f32_result, f64_result):
    """Per column: max |f32 - f64| / max |f64| (the figure of the error table)."""
    a = np.asarray(f32_result, dtype=np.float64)
    b = np.asarray(f64_result, dtype=np.float64)
    return np.abs(a - b).max(0) / np.abs(b).max(0)
