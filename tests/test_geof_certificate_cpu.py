"""The eigenvector certificate (tests/geof_certificate.py) without a GPU: the f64 oracle and the CPU
twin of the feature kernel pass it on every row of every degenerate cloud - repeated eigenvalues
included - the twin's features do not move under an exact translation, and three corrupted feature
tables are rejected (the checks have teeth)."""
import pytest
import torch

import geof_certificate as GC
from oracle import cpu_twin as T


@pytest.mark.parametrize("name,k,r", GC.CASES)
def test_inputs_are_degenerate_and_classified(name, k, r):
    """A condition on the inputs: next to no row falls between "repeated" and "simple", and the
    clouds do hold the classes they are here for."""
    ref = GC.reference(name, k, r)
    sh = GC.shares(ref.classes)
    print(f"{name} k={k} r={r}: " + " ".join(f"{c} {100 * v:.1f}%" for c, v in sh.items()))
    assert sh["mid"] <= 0.01
    total = sum(int(m.sum()) for m in ref.classes.values())
    assert total == ref.lam.shape[0]                                   # a partition
    want = {("lattice", 6): "triple", ("lattice", 45): "simple", ("floor", 8): "pair12",
            ("line", 4): "pair23", ("dup", 10): "triple", ("hex", 6): "pair12", ("hex", 18): "pair12"}
    if (name, k) in want:
        assert sh[want[(name, k)]] > 0.05
    if (name, k) == ("lattice", 45):
        assert sh["simple"] == 1.0


@pytest.mark.parametrize("name,k,r", GC.CASES)
def test_oracle_passes_the_certificate(name, k, r):
    ref = GC.reference(name, k, r)
    for k_min in ((1, 5) if name == "mixed+lattice" else (1,)):
        GC.certify(ref.oracle(k_min), ref, k_min, True, f"oracle {name} k={k} r={r} k_min={k_min}")


@pytest.mark.parametrize("name", ["floor", "hex"])
def test_oracle_passes_the_certificate_on_segment_sample_groups(name):
    xyz, val, ptr = GC.patch_groups(name)
    assert ptr.numel() == 51 and val.unique().numel() == 800
    ref = GC.GroupReference(xyz, val, ptr)
    assert GC.shares(ref.classes)["mid"] <= 0.01
    for k_min in (1, 17):
        GC.certify(ref.oracle(k_min), ref, k_min, True, f"oracle, groups of {name} k_min={k_min}")


@pytest.mark.parametrize("name,k,r", GC.CASES)
@pytest.mark.parametrize("post", [True, False])
def test_cpu_twin_passes_the_certificate(name, k, r, post):
    ref = GC.reference(name, k, r)
    for k_min in ((1, 5) if name == "mixed+lattice" else (1,)):
        f = T.point_geof(ref.xyz, ref.nn, k_min=k_min, post=post)
        GC.certify(f, ref, k_min, post, f"twin {name} k={k} r={r} k_min={k_min} post={post}")


@pytest.mark.parametrize("name,k,r", [c for c in GC.CASES if c[0] in GC.SHIFTS])
def test_cpu_twin_is_translation_invariant_bit_for_bit(name, k, r):
    """Every coordinate stays an exact f32 multiple of 0.25, so every offset and every moment sum is
    exact in f64: the features of the shifted cloud (same lists) are the unshifted ones' bit for bit."""
    ref = GC.reference(name, k, r)
    moved = ref.xyz + torch.tensor(GC.SHIFTS[name])
    assert bool(((moved * 4) == (moved * 4).round()).all())
    assert torch.equal(moved - torch.tensor(GC.SHIFTS[name]), ref.xyz)
    assert torch.equal(T.point_geof(moved, ref.nn, k_min=1), T.point_geof(ref.xyz, ref.nn, k_min=1))


def _table(ref):
    return ref.oracle(1).clone()


def test_scaled_normals_are_rejected():
    ref = GC.reference("lattice", 26, 0.6)
    f = _table(ref)
    f[:, 4:7] *= 1 + 1e-5
    with pytest.raises(AssertionError, match=r"\|n\| - 1"):
        GC.check_normal(f, ref.C, ref.lam, ref.cnt, 1, True)


@pytest.mark.parametrize("name,k,r", [("lattice", 6, 0.3), ("floor", 8, 0.4), ("hex", 18, 0.8)])
def test_second_eigenvector_as_normal_is_rejected(name, k, r):
    """On pair12 rows (l1 = l2 > l3) the normal IS unique: a vector of the repeated pair in its place is
    unit and finite, and only the residual tells."""
    ref = GC.reference(name, k, r)
    rows = ref.classes["pair12"]
    assert int(rows.sum()) > 10
    f = _table(ref)
    v = ref.V[:, :, 1].clone()
    v[v[:, 2] < 0] *= -1
    f[rows, 4:7] = v[rows]
    with pytest.raises(AssertionError, match="no eigenvector of lambda_min"):
        GC.check_normal(f, ref.C, ref.lam, ref.cnt, 1, True)
    GC.check_normal(_table(ref), ref.C, ref.lam, ref.cnt, 1, True)


def test_verticality_of_another_class_is_rejected():
    """One row's verticality replaced by the oracle's value of a row of another class: a simple row
    given a pair12 row's value, a pair12 row given a simple row's value that lies outside its family,
    an isotropic row given a flat row's value."""
    ref = GC.reference("lattice", 26, 0.6)
    cl, vr = ref.classes, ref.vref
    base = _table(ref)
    GC.check_verticality(base, ref.V, ref.lam, cl, True, ref=vr)
    simple, pair = torch.where(cl["simple"])[0], torch.where(cl["pair12"])[0]
    assert simple.numel() and pair.numel()
    # simple <- pair12
    i = int(simple[0])
    j = pair[(base[pair, 3] - base[i, 3]).abs().argmax()]
    assert abs(float(base[j, 3] - base[i, 3])) > 1e-2
    f = base.clone()
    f[i, 3] = base[j, 3]
    with pytest.raises(AssertionError, match="off the oracle"):
        GC.check_verticality(f, ref.V, ref.lam, cl, True, ref=vr)
    # pair12 <- simple
    i = int(pair[0])
    gap = torch.maximum(2 * vr["lo"][i] - base[simple, 3], base[simple, 3] - 2 * vr["hi"][i])
    j = simple[gap.argmax()]
    assert float(gap.max()) > 1e-2
    f = base.clone()
    f[i, 3] = base[j, 3]
    with pytest.raises(AssertionError, match="outside the family"):
        GC.check_verticality(f, ref.V, ref.lam, cl, True, ref=vr)
    # isotropic <- flat (the floor's verticality is 0)
    ref6 = GC.reference("lattice", 6, 0.3)
    iso = torch.where(ref6.vref["sphere"])[0]
    assert iso.numel()
    f = _table(ref6)
    f[int(iso[0]), 3] = GC.reference("floor", 8, 0.4).oracle(1)[0, 3]
    with pytest.raises(AssertionError, match="isotropic-row"):
        GC.check_verticality(f, ref6.V, ref6.lam, ref6.classes, True, ref=ref6.vref)


def test_family_is_no_single_value_and_the_grid_resolves_it():
    """The family check is needed (its range is wide on the hex plane: no single expected value) and
    its grid is fine enough: between adjacent angles the reference's curve moves by less than the
    1e-4 bar that the range is widened by, so the grid's own coarseness never doubles the slack."""
    ref = GC.reference("hex", 18, 0.8)
    fam = ref.vref["family"]
    width = (ref.vref["hi"] - ref.vref["lo"])[fam]
    step = ref.vref["slack"][fam] - 1e-4
    print(f"hex k=18: family rows {int(fam.sum())}, width up to {float(width.max()):.3f}, "
          f"largest step of the {GC.N_THETA}-point grid {float(step.max()):.2e}")
    assert float(width.max()) > 0.1
    assert float(step.max()) <= 1e-4
