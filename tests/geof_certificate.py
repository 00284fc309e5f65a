"""Certificate for the eigenVECTOR outputs of the 3x3 eigen-solver (the normal, the verticality,
scatter_pca's eigenvectors) that holds on EVERY row, repeated eigenvalues included.

On a repeated eigenvalue any basis of the eigenspace is a valid answer, so the oracle's vectors are
no expected value there.  What every valid eigen-decomposition satisfies is checked instead:

* ``check_normal``: finite, unit length, ``|| C n - lambda_min n || <= 1e-6 lambda_max`` with the
  covariance ``C`` and ``lambda_min`` from f64 torch (``eigvalsh``): no gap is needed, an eigenvector
  of a near-repeated pair still has a residual <= the gap.
* ``check_verticality``: per spectrum class - the oracle's value where it is unique, the range of the
  one-parameter family of valid bases where two eigenvalues coincide, the range over all orthonormal
  bases where all three do.

The 1e-6 bars are derived, not measured: the device solves in f64 (Jacobi stops at an off-diagonal
sum <= 1e-18 of the trace) and stores f32, so ``|| dn || <= sqrt(3) 2^-24 ~ 1e-7``, the length is off
by at most that and the residual by at most ``lambda_max 1e-7``; 1e-6 is about 10 x that.

Plain f64 torch / numpy; imported by the CPU test (oracle and CPU twin through it, corrupted tables
rejected) and by the GPU test (every consumer of eigh3 / finish_features)."""
import functools
import math

import torch

REPEATED = 1e-12        # gap <= REPEATED * lambda_1: the two eigenvalues coincide
SIMPLE = 1e-3           # gap >  SIMPLE * lambda_1: well separated (the suite's existing bar)
N_THETA = 16385         # angles of the family grid on [0, pi / 2]
SCAL = [0, 1, 2, 7, 8, 10]


# ---- covariances ---------------------------------------------------------------------------------
def _finish_cov(d, valid, cnt):
    """d [G, m, 3] f64 offsets from a per-group origin (0 where not valid) -> population covariance
    E[d d^T] - E[d] E[d]^T, symmetrised, and eigvalsh of it."""
    c = cnt.clamp(min=1).double()
    d = d * valid.unsqueeze(-1)
    m = d.sum(1) / c.view(-1, 1)
    S = torch.einsum("gki,gkj->gij", d, d) / c.view(-1, 1, 1)
    C = S - m.unsqueeze(2) * m.unsqueeze(1)
    C = 0.5 * (C + C.transpose(1, 2))
    return C, torch.linalg.eigvalsh(C)


def covariances(xyz_f32, nbr):
    """Per row the population covariance (f64) of the point itself plus its valid (>= 0) entries of
    ``nbr`` [N, k], about the point itself, from the f32 coordinates cast to f64.
    Returns ``(C [N,3,3], cnt [N], lam [N,3] ascending = eigvalsh(C))``."""
    x = xyz_f32.detach().cpu().to(torch.float32).double()
    nbr = nbr.detach().cpu().long()
    valid = nbr >= 0
    d = x[nbr.clamp(min=0)] - x.unsqueeze(1)
    cnt = valid.sum(1) + 1                   # the point itself: d = 0
    C, lam = _finish_cov(d, valid, cnt)
    return C, cnt, lam


def covariances_csr(xyz_f32, val, ptr):
    """The same for groups ``val[ptr[g] : ptr[g + 1]]`` that are no neighbourhood of a row (segment
    samples, scatter_pca groups): about the group's first entry - in f64 any origin gives the same
    covariance up to rounding.  An empty group has cnt = 0 and C = 0."""
    x = xyz_f32.detach().cpu().to(torch.float32).double()
    val, ptr = val.detach().cpu().long(), ptr.detach().cpu().long()
    size = ptr[1:] - ptr[:-1]
    G, m = size.numel(), max(int(size.max()) if size.numel() else 0, 1)
    col = torch.arange(m).view(1, -1)
    valid = col < size.view(-1, 1)
    pos = (ptr[:-1].view(-1, 1) + col).clamp(max=max(val.numel() - 1, 0))
    idx = val[pos] if val.numel() else torch.zeros((G, m), dtype=torch.long)
    valid = valid & (idx >= 0)
    p = x[idx.clamp(min=0)]
    d = p - p[:, :1]
    C, lam = _finish_cov(d, valid, valid.sum(1))
    return C, valid.sum(1), lam


def reference_eigh(C):
    """f64 ``torch.linalg.eigh`` of the certificate covariance: (lam ascending, V with the
    eigenvectors in its columns) - ONE valid decomposition, the seed of the families below."""
    return torch.linalg.eigh(C)


# ---- spectrum classes ----------------------------------------------------------------------------
def classify(lam):
    """lam [N,3] ascending.  With l1 >= l2 >= l3: a gap <= 1e-12 l1 counts as repeated, > 1e-3 l1 as
    simple.  Masks: ``simple``, ``pair12`` (l1 = l2 > l3), ``pair23`` (l1 > l2 = l3), ``triple`` (all
    equal, zero covariance included), ``mid`` (anything else)."""
    l1, l2, l3 = lam[:, 2], lam[:, 1], lam[:, 0]
    g12, g23 = l1 - l2, l2 - l3
    rep12, rep23 = g12 <= REPEATED * l1, g23 <= REPEATED * l1
    sim12, sim23 = g12 > SIMPLE * l1, g23 > SIMPLE * l1
    out = {"simple": sim12 & sim23, "pair12": rep12 & sim23, "pair23": sim12 & rep23,
           "triple": rep12 & rep23}
    out["mid"] = ~(out["simple"] | out["pair12"] | out["pair23"] | out["triple"])
    return out


def shares(classes):
    return {k: float(v.double().mean()) if v.numel() else 0.0 for k, v in classes.items()}


# ---- the normal ----------------------------------------------------------------------------------
def check_normal(f, C, lam, cnt, k_min, post):
    """Every row with ``cnt >= k_min``, no class excluded: the normal (columns 4-6) is finite, of unit
    length within 1e-6, an eigenvector of ``C`` for ``lambda_min`` with a residual <= 1e-6
    ``lambda_max``, and with ``post`` in the z >= 0 half-space.  Rows with ``cnt < k_min``: all zeros.
    Returns the figures it asserted on."""
    f = f.detach().cpu().double()
    on = cnt >= k_min
    assert bool((f[~on] == 0).all()), "a neighbourhood smaller than k_min is not all zeros"
    n = f[on][:, 4:7]
    assert bool(torch.isfinite(n).all()), "non-finite normal"
    C, lam = C[on], lam[on]
    unit = (n.norm(dim=1) - 1).abs()
    res = (torch.einsum("nij,nj->ni", C, n) - lam[:, :1] * n).norm(dim=1)
    lmax = lam[:, 2].clamp(min=0)
    rel = torch.where(lmax > 0, res / lmax.clamp(min=1e-300), torch.zeros_like(res))
    stats = {"rows": int(on.sum()), "unit": float(unit.max()) if unit.numel() else 0.0,
             "residual": float(rel.max()) if rel.numel() else 0.0}
    assert stats["unit"] <= 1e-6, f"| |n| - 1 | = {stats['unit']:.3e}"
    bad = res > 1e-6 * lmax
    assert not bool(bad.any()), \
        f"{int(bad.sum())} normals are no eigenvector of lambda_min: residual / lambda_max up to " \
        f"{stats['residual']:.3e} (zero-covariance rows with a residual: {int((bad & (lmax <= 0)).sum())})"
    if post:
        assert bool((n[:, 2] >= 0).all()), "post-processed normal with n_z < 0"
    return stats


# ---- the verticality -----------------------------------------------------------------------------
def raw_verticality(V, lam):
    """geometry.py:308-310 on one decomposition: u_r = sum_q |V_rq| lam_q (lam clamped at 0),
    verticality = u_z / (|u| + 1e-8)."""
    u = (V.abs() * lam.clamp(min=0).unsqueeze(1)).sum(2)
    return u[:, 2] / (u.norm(dim=1) + 1e-8)


def family_bounds(V, lam, cols, n_theta=N_THETA, chunk=48):
    """All valid bases of a repeated pair: the oracle's two eigenvectors ``cols`` rotated by theta in
    [0, pi / 2] (the verticality has period pi / 2 there: a quarter turn swaps the two vectors up to
    sign, which |.| and the equal weights do not see).  Returns per row (min, max, largest difference
    between adjacent grid points) of the verticality over the grid - from the reference alone."""
    a, b = cols
    c = 3 - a - b
    w = lam.clamp(min=0)
    th = torch.linspace(0, math.pi / 2, n_theta, dtype=torch.float64)
    co, si = th.cos().view(1, -1, 1), th.sin().view(1, -1, 1)
    lo, hi, step = [], [], []
    for s in range(0, V.shape[0], chunk):
        v, ww = V[s:s + chunk], w[s:s + chunk]
        va, vb, vc = v[:, :, a].unsqueeze(1), v[:, :, b].unsqueeze(1), v[:, :, c].unsqueeze(1)
        u = (co * va + si * vb).abs() * ww[:, a].view(-1, 1, 1) \
            + (co * vb - si * va).abs() * ww[:, b].view(-1, 1, 1) + vc.abs() * ww[:, c].view(-1, 1, 1)
        vert = u[:, :, 2] / (u.norm(dim=2) + 1e-8)
        lo.append(vert.min(1).values)
        hi.append(vert.max(1).values)
        step.append((vert[:, 1:] - vert[:, :-1]).abs().max(1).values)
    z = torch.zeros(0, dtype=torch.float64)
    return (torch.cat(lo) if lo else z, torch.cat(hi) if hi else z, torch.cat(step) if step else z)


def verticality_reference(V_ref, lam, classes):
    """Everything ``check_verticality`` needs that comes from the reference alone (compute once per
    cloud, share): the oracle's raw verticality, which rows have a unique value, and the family
    range (lo, hi, slack) of the rows that have none."""
    n = lam.shape[0]
    l1 = lam[:, 2]
    zero23 = classes["pair23"] & (lam[:, 1] <= REPEATED * l1)        # l2 = l3 = 0: weights 0
    zero_cov = classes["triple"] & (l1 <= 0)
    unique = classes["simple"] | zero23 | zero_cov
    fam12 = classes["pair12"]
    fam23 = classes["pair23"] & ~zero23
    lo = torch.full((n,), float("nan"), dtype=torch.float64)
    hi, slack = lo.clone(), lo.clone()
    for mask, cols in ((fam12, (1, 2)), (fam23, (0, 1))):
        if mask.any():
            a, b, s = family_bounds(V_ref[mask], lam[mask], cols)
            lo[mask], hi[mask], slack[mask] = a, b, 1e-4 + s
    return {"vert": raw_verticality(V_ref, lam), "unique": unique, "family": fam12 | fam23,
            "sphere": classes["triple"] & ~zero_cov, "lo": lo, "hi": hi, "slack": slack}


def check_verticality(f, V_ref, lam, classes, post, active=None, ref=None):
    """Column 3 by spectrum class (``active``: the rows that hold features, default all; ``ref``: a
    shared ``verticality_reference``):

    * simple rows, l2 = l3 = 0 rows and zero-covariance rows: the value is unique -> within 1e-4 of
      the oracle's (0 for zero covariance);
    * pair12 rows and pair23 rows with l2 > 0: inside the [min, max] of the family of valid bases,
      widened by 1e-4 + the largest step between adjacent grid points of the reference's own curve;
    * triple rows with lambda > 0: raw value in [1/sqrt(7), sqrt(3)/sqrt(5)] (every sum_q |V_rq| of
      an orthonormal matrix lies in [1, sqrt(3)]), widened by 1e-6;
    * every row: finite, raw value in [0, 1];  ``post``: all bounds doubled;
    * mid rows: left out of the class checks."""
    if ref is None:
        ref = verticality_reference(V_ref, lam, classes)
    v = f.detach().cpu().double()[:, 3]
    on = torch.ones_like(v, dtype=torch.bool) if active is None else active
    scale = 2.0 if post else 1.0
    assert bool(torch.isfinite(v[on]).all()), "non-finite verticality"
    assert bool(((v[on] >= 0) & (v[on] <= scale)).all()), "raw verticality outside [0, 1]"
    uq = on & ref["unique"]
    err = (v[uq] - scale * ref["vert"][uq]).abs()
    stats = {"unique_rows": int(uq.sum()), "unique_err": float(err.max()) if err.numel() else 0.0}
    assert stats["unique_err"] <= 1e-4, f"verticality off the oracle by {stats['unique_err']:.3e}"
    fam = on & ref["family"]
    lo, hi, sl = scale * ref["lo"][fam], scale * ref["hi"][fam], scale * ref["slack"][fam]
    out = torch.maximum(lo - sl - v[fam], v[fam] - hi - sl).clamp(min=0)
    stats["family_rows"] = int(fam.sum())
    stats["family_width"] = float((hi - lo).max()) if lo.numel() else 0.0
    stats["family_step"] = float((sl.max() - scale * 1e-4)) if sl.numel() else 0.0
    assert not bool((out > 0).any()), \
        f"{int((out > 0).sum())} verticalities outside the family of valid bases by up to {float(out.max()):.3e}"
    sp = on & ref["sphere"]
    stats["sphere_rows"] = int(sp.sum())
    b0, b1 = scale / math.sqrt(7.0) - 1e-6, scale * math.sqrt(3.0 / 5.0) + 1e-6
    assert bool(((v[sp] >= b0) & (v[sp] <= b1)).all()), "isotropic-row verticality outside its bounds"
    stats["checked_rows"] = stats["unique_rows"] + stats["family_rows"] + stats["sphere_rows"]
    return stats


# ---- scatter_pca's eigenvectors ------------------------------------------------------------------
def check_eigenbasis(w, V, C, lam):
    """Full decomposition of every group: columns orthonormal within 1e-6, ``|C V - V diag(w)| <=
    1e-6 lambda_max``, w ascending and >= 0, ``|w - eigvalsh(C)| <= 1e-5 max(lambda_max, 1e-6)``."""
    w, V = w.detach().cpu().double(), V.detach().cpu().double()
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(V).all())
    eye = torch.eye(3, dtype=torch.float64)
    orth = (V.transpose(1, 2) @ V - eye).abs().flatten(1).max(1).values
    res = (C @ V - V * w.unsqueeze(1)).abs().flatten(1).max(1).values
    lmax = lam[:, 2].clamp(min=0)
    rel = torch.where(lmax > 0, res / lmax.clamp(min=1e-300), torch.zeros_like(res))
    stats = {"rows": int(w.shape[0]), "orth": float(orth.max()), "residual": float(rel.max())}
    assert stats["orth"] <= 1e-6, f"max |V^T V - I| = {stats['orth']:.3e}"
    assert bool((res <= 1e-6 * lmax).all()), f"max |C V - V w| / lambda_max = {stats['residual']:.3e}"
    assert bool((w[:, 1:] >= w[:, :-1]).all()) and bool((w >= 0).all())
    assert bool(((w - lam.clamp(min=0)).abs() <= 1e-5 * lmax.clamp(min=1e-6).view(-1, 1)).all())
    return stats


# ---- the clouds ----------------------------------------------------------------------------------
# name -> [(k neighbours besides the point itself, radius)]; the spectrum classes of each, from the f64
# oracle, are printed by the tests
CASES = [("lattice", 26, 0.6), ("lattice", 6, 0.3), ("lattice", 45, 10.0),
         ("floor", 8, 0.4), ("floor", 4, 0.3), ("line", 4, 0.3), ("dup", 10, 1.0),
         ("hex", 6, 0.4), ("hex", 18, 0.8), ("mixed+lattice", 20, 0.35)]
SHIFTS = {"lattice": (5000.0, -3000.0, 100.0), "floor": (5000.0, -3000.0, 100.0),
          "hex": (4096.0, -2048.0, 512.0)}


@functools.lru_cache(maxsize=None)
def clouds():
    from test_neighbors_gpu import _clouds
    base = _clouds()
    g = torch.Generator().manual_seed(77)
    ax = torch.arange(40).float() * 0.25
    floor = torch.stack(torch.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    floor = torch.cat((floor, torch.full((floor.shape[0], 1), 1.5)), 1)        # one layer, z = 1.5
    i = torch.arange(300).float()
    # 300 points 0.125 apart in x, rising 0.0625 per step: exactly collinear in f32 (l2 = l3 = 0), and
    # oblique, so that the verticality of the one non-zero direction is neither 0 nor 1
    line = torch.stack((i * 0.125 + 2.0, torch.full_like(i, 3.0), i * 0.0625 + 1.0), 1)
    dup = torch.tensor([[1.25, -2.5, 0.75]]).repeat(40, 1)
    ij = torch.arange(-20, 20).float()
    a, b = torch.meshgrid(ij, ij, indexing="ij")
    hexp = torch.stack((a, b, -a - b), -1).reshape(-1, 3) * 0.25 + 8.0         # the plane x + y + z = 24
    hexp = hexp[torch.randperm(hexp.shape[0], generator=g)]
    mixed_lattice = torch.cat((base["mixed"], base["lattice"] + torch.tensor([20.0, 0.0, 0.0])))
    out = {"lattice": base["lattice"], "floor": floor, "line": line, "dup": dup, "hex": hexp,
           "mixed+lattice": mixed_lattice}
    assert all(v.shape[0] <= 13000 for v in out.values())
    return out


def patch_groups(name):
    """50 groups, each the 16 points of a 4 x 4 patch of the floor / the hex plane, in shuffled
    order: the segment-sample use of the CSR entry (no group is the neighbourhood of its row, the
    origin of the moments is the group's first entry)."""
    xyz = clouds()[name]
    ab = ((xyz[:, :2] - (8.0 if name == "hex" else 0.0)) / 0.25).round().long()
    ab -= ab.min(0).values
    lookup = torch.full((40, 40), -1, dtype=torch.long)
    lookup[ab[:, 0], ab[:, 1]] = torch.arange(xyz.shape[0])
    assert bool((lookup >= 0).all())
    g = torch.Generator().manual_seed(9)
    groups = []
    for p in range(50):
        a0, b0 = (p % 9) * 4, (p // 9) * 4
        idx = lookup[a0:a0 + 4, b0:b0 + 4].reshape(-1)
        groups.append(idx[torch.randperm(16, generator=g)])
    return xyz, torch.cat(groups), torch.arange(51) * 16


class Reference:
    """Everything about one (cloud, k, r) that the checks share, computed once from f64 alone."""

    def __init__(self, name, k, r):
        from oracle import spt_oracle as O
        self.name, self.k, self.r = name, k, r
        self.xyz = clouds()[name]
        dist, idx = O.frnn_grid_points(self.xyz, self.xyz, k + 1, r)
        self.nn, self.dist = idx[:, 1:].contiguous(), dist[:, 1:].contiguous()
        self.C, self.cnt, self.lam = covariances(self.xyz, self.nn)
        _, self.V = reference_eigh(self.C)
        self.classes = classify(self.lam)
        self.vref = verticality_reference(self.V, self.lam, self.classes)
        self._oracle = {}

    def oracle(self, k_min):
        if k_min not in self._oracle:
            from oracle import spt_oracle as O
            self._oracle[k_min] = O.geometric_features(self.xyz.double(), self.nn, k_min=k_min)
        return self._oracle[k_min]



class GroupReference:
    """The same for CSR groups that are no neighbourhood of their own row (``add_self=False``)."""

    def __init__(self, xyz, val, ptr):
        from oracle import spt_oracle as O
        self.xyz = xyz
        self.C, self.cnt, self.lam = covariances_csr(xyz, val, ptr)
        _, self.V = reference_eigh(self.C)
        self.classes = classify(self.lam)
        self.vref = verticality_reference(self.V, self.lam, self.classes)
        size = ptr[1:] - ptr[:-1]
        dense = torch.full((size.numel(), int(size.max())), -1, dtype=torch.long)
        dense[torch.arange(dense.shape[1]).view(1, -1) < size.view(-1, 1)] = val
        self._dense, self._O = dense, O

    def oracle(self, k_min):
        return self._O.geometric_features(self.xyz.double(), self._dense, k_min=k_min,
                                          add_self_as_neighbor=False)


def unpost(f):
    """The oracle's table without the tail of geometric_features (verticality * 2; the flip of the
    normal cannot be undone, and the sign of the normal is never compared)."""
    f = f.clone()
    f[:, 3] /= 2
    return f


@functools.lru_cache(maxsize=None)
def reference(name, k, r):
    return Reference(name, k, r)


def check_eigenvalue_columns(f, ref_f, cnt, lam, k_min):
    """Columns built from eigenVALUES against the oracle: [0, 1, 2, 7, 8, 10] within 1e-4; the volume
    (column 9) within 1e-4 on generic rows and 1e-3 on rank-deficient ones - cbrt(l1 l2 l3 + 1e-9)
    has slope 3e5 at 0, so where l3 = 0 in exact arithmetic (fewer than 4 points, or a flat / straight
    neighbourhood: lambda_min <= 1e-12 lambda_max in the f64 reference) a rounding of 1e-16 in an
    eigenvalue moves it by 3e-4 in any implementation."""
    f = f.detach().cpu().double()
    err = float((f[:, SCAL] - ref_f[:, SCAL]).abs().max())
    assert err <= 1e-4, f"eigenvalue columns off the oracle by {err:.3e}"
    deficient = (cnt < 4) | (lam[:, 0] <= REPEATED * lam[:, 2]) | (cnt < k_min)
    e9 = (f[:, 9] - ref_f[:, 9]).abs()
    g = float(e9[~deficient].max()) if (~deficient).any() else 0.0
    d = float(e9[deficient].max()) if deficient.any() else 0.0
    assert g <= 1e-4 and d <= 1e-3, (g, d)
    return {"scal": err, "vol_generic": g, "vol_deficient": d}


def certify(f, ref, k_min, post, label, C=None, cnt=None, lam=None, check_values=True):
    """The whole certificate of one feature table of ``ref``'s cloud; prints the figures."""
    C = ref.C if C is None else C
    cnt = ref.cnt if cnt is None else cnt
    lam = ref.lam if lam is None else lam
    sn = check_normal(f, C, lam, cnt, k_min, post)
    sv = check_verticality(f, ref.V, lam, ref.classes, post, active=cnt >= k_min, ref=ref.vref)
    se = {}
    if check_values:
        o = ref.oracle(k_min)
        se = check_eigenvalue_columns(f, o if post else unpost(o), cnt, lam, k_min)
    sh = shares(ref.classes)
    print(f"{label}: rows {sn['rows']}/{lam.shape[0]}  classes " +
          " ".join(f"{k} {100 * v:.1f}%" for k, v in sh.items()) +
          f"  max||n|-1| {sn['unit']:.2e}  max residual/lmax {sn['residual']:.2e}"
          f"  verticality: unique {sv['unique_rows']} (err {sv['unique_err']:.2e})"
          f" family {sv['family_rows']} (width {sv['family_width']:.3f}, step {sv['family_step']:.1e})"
          f" isotropic {sv['sphere_rows']}" + (f"  eigenvalue columns {se['scal']:.2e}" if se else ""))
    return sn, sv
