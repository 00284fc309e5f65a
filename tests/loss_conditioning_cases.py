"""Cases, float64 references, bars and two host twins for the softmax criteria of csrc/loss.hip
(``ops.cross_entropy`` plain and class-weighted, ``ops.histogram_loss`` in both modes) under
logits whose log-sum-exp is large: confident, wide and shifted rows.  Shared by
tests/test_loss_conditioning_cpu.py (no GPU: the twins against the bars) and
tests/test_loss_conditioning_gpu.py (the kernels against the same bars); nothing here touches a
device unless ``run`` is handed one.

Bars.  A sound f32 evaluation of a softmax row does C - 1 sequential f32 adds for z = sum exp(v - m),
each ``expf`` within 2 ulp, one division and one final rounding, so with S_r the weight of the row
(1 for the plain CE, w[t] in index / dominant mode, sum_c h w in histogram mode):

* gradient, per element of the un-normalised row S_r softmax - h w:  (C + 5) 2^-24 S_r, which is
  exactly 0 on a row that does not count (ignored, void-dominant, empty);
* loss:  (C + 12) 2^-24 W + 2^-23 |ref|, W = max_r S_r / den * rows (1 for the plain CE, a mean of
  row terms).  A worst case of every row at once: row errors average out, so this bar is loose and
  the gradient bar is the one that tells a sound evaluation from an unsound one.

Neither bar knows |logsumexp|: softmax is invariant under a shift of the row, and so is the error
of an evaluation that subtracts the row's maximum before anything is rounded."""
import functools

import numpy as np
import torch

KINDS = ("x3", "x30", "conf20", "mix", "off+1000", "off-3e4", "huge")
ROWS = (257, 4099)
CLASSES = (1, 2, 13, 16, 17, 32)            # 16 | 17: the seam of the kernels' CMAX template
ROUTES = ("plain", "index", "dominant", "histogram")
MASKS = ("target", "row")                   # -inf at row 0's target class / over the whole of row 0
EPS = 2.0 ** -24
NEG_INF = float("-inf")


def _generator(kind, rows, C, seed, salt):
    return torch.Generator().manual_seed((((seed * 8 + KINDS.index(kind)) * 8192 + rows) * 64 + C) * 4 + salt)


@functools.lru_cache(maxsize=None)
def logits(kind, rows, C, seed=0):
    """``(z f32 [rows, C], t int64 [rows] in [0, C), k4)``: the logits of ``kind`` around the
    labels ``t``.  From 8 rows up (and two classes) row 4 holds -inf at class ``k4 != t[4]``, a
    masked class; ``k4`` is None otherwise."""
    g = _generator(kind, rows, C, seed, 0)
    b = torch.randn(rows, C, generator=g)
    t = torch.randint(0, C, (rows,), generator=g)
    hot = torch.zeros(rows, C).scatter_(1, t[:, None], 20.0)
    if kind == "x3":
        z = b * 3
    elif kind == "x30":
        z = b * 30
    elif kind == "conf20":
        z = b + hot
    elif kind == "mix":
        z = b + hot
        z[::50] = b[::50] * 3
    elif kind == "off+1000":
        z = b * 3 + 1000
    elif kind == "off-3e4":
        z = b * 3 - 3e4
    elif kind == "huge":
        z = b * 1e37                        # exp(v - m) underflows to 0 off the maximum
    else:
        raise ValueError(kind)
    k4 = None
    if rows >= 8 and C >= 2:
        k4 = (int(t[4]) + 1) % C
        z[4, k4] = NEG_INF
    return z, t, k4


def class_weights(C, seed=0):
    """f32 [C] in [1e-3, 1e3], both ends present from two classes up."""
    g = torch.Generator().manual_seed(977 * C + seed)
    w = 10.0 ** (torch.rand(C, generator=g) * 6 - 3)
    w[0] = 1e-3
    w[C - 1] = 1e3
    return w


def index_target(kind, rows, C, seed, ignore):
    """``(t, ignore_index)``.  With ``ignore``: about one row in ten carries ignore_index = C,
    and from 8 rows up row 0 is the only counted row of its wave (rows 1 .. 63 are ignored)."""
    t = logits(kind, rows, C, seed)[1].clone()
    if not ignore:
        return t, -100
    drop = torch.rand(rows, generator=_generator(kind, rows, C, seed, 1)) < 0.1
    keep0 = int(t[0])
    t[drop] = C
    if rows >= 8:
        t[1:64] = C
    t[0] = keep0
    return t, C


def histogram_target(kind, rows, C, seed, void):
    """Sparse int64 label counts [rows, C + void].  Row 0 counts 7 points of its label (the masked
    cases hit it), row 1 is empty, rows 2 and 3 are all-void and void-dominant (with a void
    column), row 4 has no count at its masked class, row 5 counts 10^9 twice (a large S_r), row 6
    ties its first and last class (the first wins)."""
    assert rows >= 8
    z, t, k4 = logits(kind, rows, C, seed)
    g = _generator(kind, rows, C, seed, 2)
    ncols = C + int(void)
    h = torch.randint(0, 60, (rows, ncols), generator=g) * (torch.rand(rows, ncols, generator=g) < 0.3)
    h[0] = 0
    h[0, t[0]] = 7
    h[1] = 0
    if void:
        h[2] = 0
        h[2, C] = 11
        h[3, C] = h[3].max() + 1
        h[4, C] = 0
    if k4 is not None:
        h[4, k4] = 0
    h[4, t[4]] += 1
    h[5] = 0
    h[5, 0] = h[5, C - 1] = 10 ** 9
    h[6] = 0
    h[6, 0] = h[6, C - 1] = 7
    return h


def reference(route, z, target, w, ignore_index, with_grad=True):
    """float64 on the host: ``loss`` (0-d), ``grad`` [rows, C] = S_r softmax - h w (un-normalised:
    the kernels' gradient times den / gout), ``S`` [rows], ``den`` and ``W`` of the loss bar.
    Plain and index mode: torch's cross_entropy and its autograd; dominant and histogram: the
    closed forms of tests/test_hist_loss_gpu.py, a zero count kept out of the product so that it
    meets a masked logit as 0 and not as 0 * inf."""
    F = torch.nn.functional
    rows, C = z.shape
    zd = z.double()
    wd = torch.ones(C, dtype=torch.float64) if route == "plain" else w.double()
    grad = None
    if route in ("plain", "index"):
        valid = target != ignore_index
        S = torch.where(valid, wd[target.clamp(max=C - 1)], torch.zeros((), dtype=torch.float64))
        den = S.sum()
        zr = zd.clone().requires_grad_(with_grad)
        loss = F.cross_entropy(zr, target, weight=None if route == "plain" else wd, ignore_index=ignore_index)
        if with_grad:
            grad = torch.autograd.grad(loss, zr)[0] * den
        loss = loss.detach()
    elif route == "dominant":
        td = target.argmax(dim=1)
        valid = td < C
        S = torch.where(valid, wd[td.clamp(max=C - 1)], torch.zeros((), dtype=torch.float64))
        den = S.sum()
        loss = F.cross_entropy(zd, td, weight=wd, ignore_index=C)
        if with_grad:
            hw = torch.zeros(rows, C + 1, dtype=torch.float64).scatter_(1, td[:, None], 1.0)[:, :C] * S[:, None]
            grad = S[:, None] * torch.softmax(zd, dim=1) - hw
    elif route == "histogram":
        hw = target[:, :C].double() * wd
        lse = torch.logsumexp(zd, dim=1)
        den = target.sum().double()
        loss = torch.where(hw != 0, hw * (lse[:, None] - zd), torch.zeros((), dtype=torch.float64)).sum() / den
        S = hw.sum(dim=1)
        if with_grad:
            grad = S[:, None] * torch.softmax(zd, dim=1) - hw
    else:
        raise ValueError(route)
    W = 1.0 if route == "plain" else float(S.max() / den) * rows
    return dict(loss=loss, grad=grad, S=S, den=float(den), W=W)


@functools.lru_cache(maxsize=None)
def case(route, kind, rows, C, seed=0, flag=False, mask=None):
    """Inputs and reference of one case, built once and shared (nobody writes into them).
    ``flag``: ignore_index rows (plain, index) or a void column (dominant, histogram).
    ``mask``: None, or one of MASKS applied to row 0, which counts in every route."""
    z, t, k4 = logits(kind, rows, C, seed)
    w = None if route == "plain" else class_weights(C, seed)
    if route in ("plain", "index"):
        target, ii = index_target(kind, rows, C, seed, flag)
    else:
        target, ii = histogram_target(kind, rows, C, seed, flag), -100
    if mask is not None:
        z = z.clone()
        if mask == "target":
            z[0, t[0]] = NEG_INF
        else:
            z[0] = NEG_INF
    ref = reference(route, z, target, w, ii, with_grad=mask is None)
    return dict(route=route, kind=kind, rows=rows, C=C, z=z, target=target, w=w, ignore_index=ii,
                k4=k4, label=t, **ref)


def grad_bar(c):
    return (c["C"] + 5) * EPS * c["S"][:, None]


def loss_bar(c):
    return (c["C"] + 12) * EPS * c["W"] + 2 * EPS * abs(float(c["loss"]))


def ratios(c, loss, grad, gout=1.0):
    """``(gradient error / bar, loss error / bar, zero_ok)`` of a result against the case's
    reference.  ``grad`` is as the kernels return it, (S_r softmax - h w) gout / den, any float
    dtype; the ratio is the largest over the elements of the rows that count, and ``zero_ok``
    says that every element of the other rows is exactly 0 (their bar)."""
    gn = torch.as_tensor(grad).double() * (c["den"] / gout)
    err = (gn - c["grad"]).abs()
    counts = c["S"] > 0
    zero_ok = bool((torch.as_tensor(grad)[~counts] == 0).all())
    gr = float((err[counts] / grad_bar(c)[counts]).max()) if bool(counts.any()) else 0.0
    lr = abs(float(loss) - float(c["loss"])) / loss_bar(c)
    return gr, lr, zero_ok


def same_kind(a, b):
    """Both NaN, both the same infinity, or both finite."""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return a == b
    return True


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run(dev, c, gout=1.0):
    """One forward and backward of the case's route on ``dev``: ``(loss, grad)`` on the host."""
    from superpoint_transformer_amd import ops
    z = c["z"].clone().to(dev).requires_grad_()             # (a copy also when dev is the host)
    target = c["target"].to(dev)
    w = None if c["w"] is None else c["w"].to(dev)
    if c["route"] in ("plain", "index"):
        loss = ops.cross_entropy(z, target, ignore_index=c["ignore_index"], weight=w)
    else:
        loss = ops.histogram_loss(z, target, weight=w, mode=c["route"])
    assert loss.dtype == torch.float32
    grad, = torch.autograd.grad(loss, z, grad_outputs=torch.tensor(gout, device=dev))
    return loss.detach().cpu(), grad.cpu()


def line(c, flag, gr, lr):
    """The record of one measurement, as profiles/r26a_loss_conditioning_errors.txt tabulates it."""
    return (f"LCOND {c['route']:9s} {c['kind']:8s} C {c['C']:2d} rows {c['rows']:4d} flag {int(flag)} "
            f"grad err/bar {gr:10.4g}  loss err/bar {lr:10.4g}")


# ---- the plain CE's arithmetic on the host, operation by operation in f32 --------------------------
def _row_terms(c):
    """m, e = expf(v - m), z by sequential f32 adds in column order, the picked logit, the mask of
    counted rows and the one-hot labels: what both twins (and both generations of ce_*_kernel)
    share."""
    v = c["z"].numpy()
    t = c["target"].numpy()
    assert v.dtype == np.float32
    rows, C = v.shape
    valid = t != c["ignore_index"]
    tc = np.where(valid, t, 0)
    m = v.max(axis=1)
    e = np.exp(v - m[:, None])
    z = np.zeros(rows, dtype=np.float32)
    for k in range(C):
        z = z + e[:, k]
    assert e.dtype == np.float32 and z.dtype == np.float32
    picked = v[np.arange(rows), tc]
    onehot = np.zeros((rows, C), dtype=np.float32)
    onehot[np.arange(rows), tc] = 1
    return v, m, e, z, picked, valid, onehot


def _finish(row_loss, g, valid):
    """The mean over the counted rows in f64, rounded to f32 once; 0 on the other rows."""
    loss = np.float32(row_loss[valid].astype(np.float64).sum() / valid.sum())
    return loss, torch.from_numpy(np.where(valid[:, None], g, 0).astype(np.float64))


def old_arithmetic(c):
    """The plain CE as first written: l = f32(m + logf(z)) stored, the row term f32(l - picked),
    p = expf(v - l).  ``(loss f32, un-normalised gradient)``: the gradient before its f32
    product with gout / count, which would add up to 2^-24 relative."""
    v, m, e, z, picked, valid, onehot = _row_terms(c)
    l = m + np.log(z)
    assert l.dtype == np.float32
    p = np.exp(v - l[:, None])
    return _finish(l - picked, p - onehot, valid)


def sound_arithmetic(c):
    """The arithmetic of hl_*_kernel: the row term f64(logf(z)) + (f64(m) - f64(picked)),
    p = f64(e_c) / f64(z), the gradient rounded to f32 once."""
    v, m, e, z, picked, valid, onehot = _row_terms(c)
    row = np.log(z).astype(np.float64) + (m.astype(np.float64) - picked.astype(np.float64))
    p = e.astype(np.float64) / z.astype(np.float64)[:, None]
    return _finish(row, (p - onehot).astype(np.float32), valid)
