"""GPU: the eigenVECTOR outputs of eigh3 / finish_features on repeated-eigenvalue neighbourhoods.

Voxelised clouds are lattices: a floor or a wall has l1 = l2 by symmetry, a cable l2 = l3 = 0, and the
tests that compare columns 3-6 with the oracle skip exactly those rows.  Here every row of every
consumer is checked with what holds for ANY valid eigen-decomposition (tests/geof_certificate.py):
the normal is a unit eigenvector of lambda_min (residual against the f64 covariance), the verticality
lies in the family of values the valid bases allow, scatter_pca returns an orthonormal eigenbasis.
The eigenvalue columns are compared with the oracle in every test, so that each stands on its own.

Consumers: geometric_features (dense, row-pitch and CSR entries, segment-sample groups), the features
summed inside the kNN kernel (cell path, its leftovers, wave per query), scatter_pca.  Under a
translation that keeps every coordinate an exact multiple of 0.25 the one-kernel entries must not
move by a bit (moments about the point, in f64)."""
import pytest
import torch

import geof_certificate as GC
from oracle import spt_oracle as O

pytestmark = pytest.mark.gpu

# (cloud, k, r, k_min): partial and empty neighbourhoods (mixed+lattice) with both k_min
PARAMS = [c + (1,) for c in GC.CASES] + [("mixed+lattice", 20, 0.35, 5)]
SHIFTED = [c for c in GC.CASES if c[0] in GC.SHIFTS]


def _label(path, name, k, r, k_min, **kw):
    return f"{path} {name} k={k} r={r} k_min={k_min} " + " ".join(f"{a}={b}" for a, b in kw.items())


@pytest.mark.parametrize("name,k,r,k_min", PARAMS)
@pytest.mark.parametrize("raw", [False, True])
def test_dense_entry_on_every_row(name, k, r, k_min, raw, dev):
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    f = NB.geometric_features(ref.xyz.to(dev), ref.nn.to(dev), k_min=k_min, raw=raw, order=False)
    GC.certify(f, ref, k_min, not raw, _label("dense", name, k, r, k_min, raw=raw))


@pytest.mark.parametrize("name,k,r,k_min", PARAMS)
def test_row_pitch_entry_on_every_row(name, k, r, k_min, dev):
    """``nn`` as a column slice of a [N, k + 1] table (what knn_1 hands out): read in place."""
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    n = ref.xyz.shape[0]
    table = torch.cat((torch.arange(n).view(-1, 1), ref.nn), dim=1).to(dev)
    nn = table[:, 1:]
    assert not nn.is_contiguous()
    p = ref.xyz.to(dev)
    for raw in (False, True):
        f = NB.geometric_features(p, nn, k_min=k_min, raw=raw, order=False)
        GC.certify(f, ref, k_min, not raw, _label("row-pitch", name, k, r, k_min, raw=raw))
        assert torch.equal(f, NB.geometric_features(p, nn.contiguous(), k_min=k_min, raw=raw, order=False))


@pytest.mark.parametrize("name,k,r,k_min", PARAMS)
def test_csr_entry_with_the_point_in_its_list(name, k, r, k_min, dev):
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    n = ref.xyz.shape[0]
    ptr, val, _ = O.neighbors_dense_to_csr(torch.cat((torch.arange(n).view(-1, 1), ref.nn), dim=1))
    p = ref.xyz.to(dev)
    f = NB.geometric_features_csr(p, val.to(dev), ptr.to(dev), k_min=k_min, add_self=False, raw=False)
    GC.certify(f, ref, k_min, True, _label("csr", name, k, r, k_min))
    assert torch.equal(f, NB.geometric_features(p, ref.nn.to(dev), k_min=k_min, order=False))


@pytest.mark.parametrize("name", ["floor", "hex"])
@pytest.mark.parametrize("raw", [False, True])
def test_csr_entry_on_segment_sample_groups(name, raw, dev):
    from superpoint_transformer_amd import neighbors as NB
    xyz, val, ptr = GC.patch_groups(name)
    ref = GC.GroupReference(xyz, val, ptr)
    assert GC.shares(ref.classes)["mid"] <= 0.01
    for k_min in (1, 17):                          # 17: every group is too small -> all zeros
        f = NB.geometric_features_csr(xyz.to(dev), val.to(dev), ptr.to(dev), k_min=k_min,
                                      add_self=False, raw=raw)
        assert f.shape == (50, 11)
        GC.certify(f, ref, k_min, not raw, f"csr groups {name} k_min={k_min} raw={raw}")


@pytest.mark.parametrize("name,k,r,k_min", PARAMS)
@pytest.mark.parametrize("formulation", [-1, 0])
@pytest.mark.parametrize("cell", [None, 0.11, 3.7])
@pytest.mark.parametrize("raw", [False, True])
def test_features_out_of_the_knn_kernel_on_every_row(name, k, r, k_min, formulation, cell, raw, dev):
    """Cell kernel, its leftovers (cells far too fine / too coarse push queries there) and the
    wave-per-query kernel: neighbours and distances are knn_1's bit for bit (and the oracle's, whose
    lists the certificate covariance is built from), the features pass the certificate on ALL rows."""
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    p = ref.xyz.to(dev)
    nb0, d0 = NB.knn_1(p, k, r)
    nb, d, f = NB.knn_1_features(p, k, r, k_min=k_min, raw=raw, formulation=formulation, cell_size=cell)
    assert torch.equal(nb, nb0) and torch.equal(d, d0)
    assert torch.equal(nb.cpu(), ref.nn) and torch.equal(d.cpu(), ref.dist)
    GC.certify(f, ref, k_min, not raw,
               _label("knn", name, k, r, k_min, formulation=formulation, cell=cell, raw=raw))


@pytest.mark.parametrize("name,k,r", [c for c in GC.CASES if c[0] in ("lattice", "hex")])
def test_scatter_pca_eigenbasis_on_every_group(name, k, r, dev):
    """The groups are the neighbourhoods (point + neighbours) of the cloud, the group index shuffled,
    two empty groups last: on every non-empty group an orthonormal eigenbasis of its covariance."""
    from superpoint_transformer_amd import segment as SG
    ref = GC.reference(name, k, r)
    n = ref.xyz.shape[0]
    ptr, val, _ = O.neighbors_dense_to_csr(torch.cat((torch.arange(n).view(-1, 1), ref.nn), dim=1))
    gidx = torch.repeat_interleave(torch.arange(n), ptr[1:] - ptr[:-1])
    pts = ref.xyz[val]
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(1))
    w, V = SG.scatter_pca(pts[perm].to(dev), gidx[perm].to(dev), n + 2)
    w, V = w.cpu(), V.cpu()
    st = GC.check_eigenbasis(w[:n], V[:n], ref.C, ref.lam)
    sh = GC.shares(ref.classes)
    print(f"scatter_pca {name} k={k} r={r}: groups {n}  classes " +
          " ".join(f"{c} {100 * v:.1f}%" for c, v in sh.items()) +
          f"  max|VtV-I| {st['orth']:.2e}  max|CV-Vw|/lmax {st['residual']:.2e}")
    assert torch.equal(w[n:], torch.ones(2, 3))
    assert torch.equal(V[n:], torch.eye(3).expand(2, 3, 3))


def _moved(name, xyz):
    shift = torch.tensor(GC.SHIFTS[name])
    moved = xyz + shift
    assert bool(((moved * 4) == (moved * 4).round()).all())        # exact multiples of 0.25 ...
    assert torch.equal(moved - shift, xyz)                         # ... and nothing was rounded away
    return moved


@pytest.mark.parametrize("name,k,r", SHIFTED)
@pytest.mark.parametrize("raw", [False, True])
def test_translation_does_not_move_a_bit_dense_and_csr(name, k, r, raw, dev):
    """Every x_j - x_i and every moment sum is exact in f64 before and after the shift: the features
    of the same lists are equal bit for bit.  Sums about the global origin, or in f32, break this."""
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    p, q = ref.xyz.to(dev), _moved(name, ref.xyz).to(dev)
    nn = ref.nn.to(dev)
    f = NB.geometric_features(p, nn, k_min=1, raw=raw, order=False)
    fm = NB.geometric_features(q, nn, k_min=1, raw=raw, order=False)
    GC.certify(fm, ref, 1, not raw, _label("dense, shifted", name, k, r, 1, raw=raw))
    assert torch.equal(fm, f)
    n = ref.xyz.shape[0]
    ptr, val, _ = O.neighbors_dense_to_csr(torch.cat((torch.arange(n).view(-1, 1), ref.nn), dim=1))
    c = NB.geometric_features_csr(p, val.to(dev), ptr.to(dev), k_min=1, add_self=False, raw=raw)
    cm = NB.geometric_features_csr(q, val.to(dev), ptr.to(dev), k_min=1, add_self=False, raw=raw)
    assert torch.equal(cm, c) and torch.equal(cm, f)


@pytest.mark.parametrize("name,k,r", SHIFTED)
@pytest.mark.parametrize("formulation", [-1, 0])
@pytest.mark.parametrize("cell", [None, 0.11, 3.7])
def test_translation_of_the_knn_kernel_features(name, k, r, formulation, cell, dev):
    """A query may move between the cell kernel and its leftovers when the grid origin moves, so
    here: neighbours and distances bit for bit, the certificate, and the eigenvalue columns within
    1e-6 of the unshifted run."""
    from superpoint_transformer_amd import neighbors as NB
    ref = GC.reference(name, k, r)
    p, q = ref.xyz.to(dev), _moved(name, ref.xyz).to(dev)
    nb, d, f = NB.knn_1_features(p, k, r, k_min=1, formulation=formulation, cell_size=cell)
    nbm, dm, fm = NB.knn_1_features(q, k, r, k_min=1, formulation=formulation, cell_size=cell)
    assert torch.equal(nbm, nb) and torch.equal(dm, d)
    assert torch.equal(nbm.cpu(), ref.nn)
    GC.certify(fm, ref, 1, True, _label("knn, shifted", name, k, r, 1, formulation=formulation, cell=cell))
    assert float((fm[:, GC.SCAL] - f[:, GC.SCAL]).abs().max()) <= 1e-6
