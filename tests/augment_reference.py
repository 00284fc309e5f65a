"""numpy / f64 restatement of the augmentation block of the training chain: the counter-based
generator, the noise formula and every map of

    NAGJitterKey, NAGDropoutColumns, NAGDropoutRows     src/transforms/data.py:440-721
    RandomTiltAndRotate, RandomAnisotropicScale, RandomAxisFlip
                                                        src/transforms/geometry.py:28-245
    NAGColorAutoContrast, NAGColorDrop                  src/transforms/point.py:374-545

shared by tests/golden/make_golden_augment.py and the augmentation tests.  Written from the
reference and from the specification of the stream, not from the kernels; nothing is imported
from the reference or from the package.  Only ``erf`` / ``erfinv`` come from torch (f64).

The stream: ``r = rand32(seed, counter)`` is the splitmix64 finaliser
``z = seed + 0x9E3779B97F4A7C15 * (counter + 1)``, two xor-shift-multiply rounds, a last
xor-shift, the high 32 bits.  The counter of element (row, col) of an [n, c] tensor is
``row * c + col``, the counter of a row decision is ``row``.
  decision  u = (r >> 8) * 2**-24 in [0, 1), taken when u < float32(p)
  noise     u = ((r >> 8) + 0.5) * 2**-24 in (0, 1),
            clamp(sigma * sqrt(2) * erfinv(lo + u * (hi - lo)), -trunc, trunc),
            lo = 2 Phi(-trunc / sigma) - 1, hi = 2 Phi(trunc / sigma) - 1
            (torch.nn.init.trunc_normal_); trunc <= 0: lo = -1, hi = 1, no clamp.
"""
import math

import numpy as np
import torch

# max |reference f32 - f64 restatement| / max |f64| per column, the largest column, per map, on
# tests/golden/augment.npz; measured by tests/test_augment_reference_cpu.py
# (test_reference_deviation prints them) and recorded in profiles/r15a_augment_errors.txt.  The
# GPU suite allows the kernels MARGIN times this against the fixture.
REFERENCE_DEVIATION = {
    "rotate_pos": 6.65e-08,
    "rotate_normal": 8.43e-08,
    "rotate_edge": 7.51e-08,
    "scale_normal": 1.05e-07,
    "scale_edge": 5.98e-08,
    "contrast": 9.96e-08,
}
# max |f32 torch evaluation - f64| / sigma of the noise formula over 2**20 counters, per
# (sigma, trunc); the untruncated form is ill-conditioned at the tail (indicative)
NOISE_DEVIATION = {(0.03, 0.03): 2.7e-07, (0.01, 0.02): 1.4e-06, (1.0, 0.0): 4.3e-03}
MARGIN = 4.0

_M = np.uint64(0xFFFFFFFFFFFFFFFF)


def rand32(seed, counters):
    """uint64 array of values in [0, 2**32)."""
    with np.errstate(over="ignore"):
        i = np.asarray(counters).astype(np.uint64)
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * (i + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return z >> np.uint64(32)


def rand32_scalar(seed, i):
    """The same in Python integers (checks the array version)."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z = z ^ (z >> 31)
    return z >> 32


def decision_uniform(seed, counters):
    """f64 (exactly representable in f32) u in [0, 1)."""
    return (rand32(seed, counters) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def decisions(seed, counters, p):
    return decision_uniform(seed, counters) < np.float64(np.float32(p))


def noise_uniform(seed, counters):
    return ((rand32(seed, counters) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def noise_bounds(sigma, trunc):
    if trunc <= 0:
        return -1.0, 1.0
    phi = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731
    return 2.0 * phi(-trunc / sigma) - 1.0, 2.0 * phi(trunc / sigma) - 1.0


def erfinv(x):
    return torch.special.erfinv(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def noise_from_uniform(u, sigma, trunc):
    lo, hi = noise_bounds(sigma, trunc)
    z = sigma * math.sqrt(2.0) * erfinv(lo + u * (hi - lo))
    return np.clip(z, -trunc, trunc) if trunc > 0 else z


def noise(seed, counters, sigma, trunc):
    return noise_from_uniform(noise_uniform(seed, counters), sigma, trunc)


def noise_cdf(z, sigma, trunc):
    """CDF of the (truncated) normal at z."""
    z = np.asarray(z, dtype=np.float64)
    phi = 0.5 * (1.0 + torch.special.erf(torch.from_numpy(z / (sigma * math.sqrt(2.0)))).numpy())
    if trunc <= 0:
        return phi
    lo, hi = noise_bounds(sigma, trunc)
    a, b = 0.5 * (lo + 1.0), 0.5 * (hi + 1.0)
    return np.clip((phi - a) / (b - a), 0.0, 1.0)


def element_counters(n, c):
    return np.arange(n * c, dtype=np.uint64).reshape(n, c)


# ---- the maps (f64 on the f32 inputs) ---------------------------------------------------------
def jitter(x, seed, sigma, trunc):
    x = np.asarray(x, dtype=np.float64)
    x2 = x.reshape(x.shape[0], -1)
    return (x2 + noise(seed, element_counters(*x2.shape), sigma, trunc)).reshape(x.shape)


def drop_columns(x, cols):
    out = np.array(x, copy=True)
    out[:, np.asarray(cols, dtype=np.int64)] = 0
    return out


def drop_rows(x, rows):
    out = np.array(x, copy=True)
    out[np.asarray(rows, dtype=np.int64)] = 0
    return out


def dropped_rows(seed, n, p):
    return np.nonzero(decisions(seed, np.arange(n), p))[0]


def rotate(v, R):
    return np.asarray(v, dtype=np.float64) @ np.asarray(R, dtype=np.float64).T


def upward(v):
    """normal[normal[:, 2] < 0] *= -1"""
    out = np.array(v, copy=True)
    neg = out[:, 2] < 0
    out[neg] = -out[neg]
    return out


def normalize(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1e-12)


def flip(v, axis):
    out = np.array(v, copy=True)
    out[:, axis] = -out[:, axis]
    return out


def tilt_pos(pos, R):
    return rotate(pos, R)


def tilt_normal(nrm, R):
    return upward(rotate(nrm, R))


def tilt_edge(ea, R):
    out = np.asarray(ea, dtype=np.float64).copy()
    out[:, :3] = rotate(out[:, :3], R)
    return out


def scale_pos(pos, scale):
    return np.asarray(pos, dtype=np.float64) * np.asarray(scale, dtype=np.float64)


def scale_normal(nrm, scale):
    return normalize(np.asarray(nrm, dtype=np.float64) * np.asarray(scale, dtype=np.float64))


def scale_edge(ea, scale):
    s = np.asarray(scale, dtype=np.float64)
    out = np.asarray(ea, dtype=np.float64).copy()
    out[:, :3] *= s
    out[:, 3:] *= np.sqrt((s * s).sum())
    return out


def flip_pos(pos, axis):
    return flip(pos, axis)


def flip_normal(nrm, axis):
    return upward(flip(nrm, axis))


def flip_edge(ea, axis):
    return flip(ea, axis)


def contrast(c, blend, lo=None, hi=None):
    c = np.asarray(c, dtype=np.float64)
    lo = c.min(0, keepdims=True) if lo is None else np.asarray(lo, dtype=np.float64).reshape(1, 3)
    hi = c.max(0, keepdims=True) if hi is None else np.asarray(hi, dtype=np.float64).reshape(1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (1.0 - blend) * c + blend * ((c - lo) / (hi - lo))


def color_drop(c):
    return np.asarray(c) * np.zeros((), dtype=np.asarray(c).dtype)


def rodrigues(axis, theta_degrees):
    """f64 Rodrigues matrix (src/utils/geometry.py:27-39)."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = theta_degrees / 180.0 * np.pi
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def relative_deviation(a, ref):
    """max over columns of max |a - ref| / max |ref| (NaN positions must coincide and are left
    out; a column of zeros counts its absolute deviation)."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    ref = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    assert a.shape == ref.shape
    assert np.array_equal(np.isnan(a), np.isnan(ref)), "NaN positions differ"
    worst = 0.0
    for j in range(ref.shape[1]):
        ok = ~np.isnan(ref[:, j])
        if not ok.any():
            continue
        top = np.abs(ref[ok, j]).max()
        worst = max(worst, np.abs(a[ok, j] - ref[ok, j]).max() / (top if top > 0 else 1.0))
    return worst


def ks_distance(z, sigma, trunc):
    """Kolmogorov-Smirnov distance of the sample z to the analytic CDF."""
    z = np.sort(np.asarray(z, dtype=np.float64).reshape(-1))
    n = z.size
    F = noise_cdf(z, sigma, trunc)
    return max(np.abs(F - np.arange(n) / n).max(), np.abs(F - np.arange(1, n + 1) / n).max())


def lag1(z):
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    z = z - z.mean()
    return float((z[:-1] * z[1:]).sum() / (z * z).sum())
