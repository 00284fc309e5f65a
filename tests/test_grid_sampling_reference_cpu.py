"""CPU suite of ``GridSampling3D``: tests/golden/grid_sampling.npz is output of the REFERENCE'S
OWN ``GridSampling3D._process`` / ``_group_data`` (tests/golden/make_golden_grid_sampling.py).
The restatement (tests/grid_sampling_reference.py) and the package's CPU composition
(``transforms.GridSampling3D`` on CPU tensors) must both reproduce it: indices, histograms, votes,
``obj`` overlaps and coords exactly, means bit for bit, ``sub`` as the same points per voxel (the
reference's order inside a voxel comes from an unstable sort: ``canonical_sub``).

The reference's own f32 deviation from the f64 restatement, max |diff| / max |f64| over the worst
case, is measured and printed per key; the GPU suite's bound is 4 x that figure."""
import numpy as np
import pytest
import torch

import grid_sampling_reference as R


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def package_result(data):
    """A package ``Data`` -> the restatement's result layout."""
    out = {}
    for k, v in data:
        name = type(v).__name__
        if name == "Cluster":
            out[k] = (v.pointers.cpu(), v.points.cpu())
        elif name == "InstanceData":
            out[k] = tuple(t.cpu() for t in (v.pointers, v.obj, v.count, v.y))
        else:
            out[k] = v.cpu() if torch.is_tensor(v) else v
    return out


def run_package(fields, kwargs, device="cpu"):
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import GridSampling3D
    data = Data(**{k: v.clone().to(device) for k, v in fields.items()})
    t = GridSampling3D(**kwargs)
    t.shuffle = False            # the fixture's 'last' case took the identity for the shuffle
    return package_result(t(data)), t


def expected(golden, case):
    pre = case + "__"
    return {k: v for k, v in golden.items() if k.startswith(pre)}


def assert_reproduces(golden, case, result, what):
    want = expected(golden, case)
    got = R.flatten(result, case, R.CASE_KEYS[case])
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if k.endswith("__sub__points"):
            ptr = want[k.replace("points", "pointers")]
            w = R.canonical_sub(ptr, w).numpy()
            g = R.canonical_sub(ptr, g).numpy()
        assert R.bits_equal(w, g), f"{what}, {k}: differs from the reference's output"


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_reproduces_the_reference(golden, case):
    kwargs, with_batch = R.CASES[case]
    out = R.grid_sampling(R.golden_fields(golden, with_batch), **kwargs)
    assert_reproduces(golden, case, out, "restatement")


@pytest.mark.parametrize("case", list(R.CASES))
def test_cpu_composition_reproduces_the_reference(golden, case):
    kwargs, with_batch = R.CASES[case]
    out, _ = run_package(R.golden_fields(golden, with_batch), kwargs)
    assert_reproduces(golden, case, out, "package on the CPU")


def test_voxel_order_is_lexicographic(golden):
    """grid_cluster / voxel_grid + consecutive_cluster number the voxels in (batch, z, y, x)
    order - the rule the device key is built on."""
    for with_batch in (False, True):
        f = R.golden_fields(golden, with_batch)
        for size in (R.SIZE, R.FINE_SIZE):
            coords, cluster, perm = R.voxelize(f["pos"], size, f.get("batch"))
            assert torch.equal(cluster, R.lexicographic_cluster(coords, f.get("batch")))
            # the representative is the highest point index of the voxel
            best = torch.zeros(perm.numel(), dtype=torch.long)
            best.scatter_reduce_(0, cluster, torch.arange(cluster.numel()), "amax")
            assert torch.equal(perm, best)


def test_cloud_has_the_cases_the_fixture_promises(golden):
    f = R.golden_fields(golden)
    pos = f["pos"]
    assert float(pos.min()) < -1 and float(pos.max()) > 1
    q = pos / R.SIZE
    ties = (q - torch.floor(q)) == 0.5
    assert int(ties.all(dim=1).sum()) >= 300           # the half-way block
    r = torch.round(q[ties])
    assert bool((r % 2 == 0).all())                    # ties went to even
    counts = np.diff(golden["default__sub__pointers"])
    assert counts.max() >= 300 and (counts == 1).sum() >= 400
    assert int(f["y"].max()) < R.NUM_BINS and int(f["y"].min()) == 0
    assert golden["default__other"].shape == (7,)
    assert golden["batch__pos"].shape[0] > golden["default__pos"].shape[0]


def reference_deviation(golden):
    """{key: max over the mean-mode cases of max |reference f32 - f64| / max |f64|}."""
    worst = {}
    for case, (kwargs, with_batch) in R.CASES.items():
        if kwargs.get("mode", "mean") != "mean":
            continue
        m64 = R.grid_sampling(R.golden_fields(golden, with_batch), dtype=torch.float64, **kwargs)
        for k in R.MEAN_KEYS:
            name = f"{case}__{k}"
            if name in golden:
                assert m64[k].dtype == torch.float64
                worst[k] = max(worst.get(k, 0.0), R.relative_deviation(golden[name], m64[k].numpy()))
    return worst


def test_reference_f32_deviation_is_measured(golden):
    worst = reference_deviation(golden)
    assert set(worst) == set(R.MEAN_KEYS)
    print("\nreference f32 deviation from the f64 restatement (max |diff| / max |f64|, worst case):")
    for k, v in worst.items():
        print(f"  {k}: {v:.3e}")
        assert 0 <= v < 1e-5                 # an f32 mean of a few hundred values at the most
    assert worst["rgb"] > 0 and worst["intensity"] > 0     # the 320-point voxel shows


def test_groups_are_consistent_on_the_cpu(golden):
    from superpoint_transformer_amd import voxel
    f = R.golden_fields(golden, True)
    g = voxel.voxel_groups(f["pos"], R.SIZE, f["batch"])
    _, cluster, perm = R.voxelize(f["pos"], R.SIZE, f["batch"])
    assert torch.equal(g.cluster, cluster) and torch.equal(g.last, perm)
    assert torch.equal(g.order, torch.sort(cluster, stable=True).indices)
    assert torch.equal(g.coords.float(), torch.round(f["pos"] / R.SIZE)[perm])
    assert torch.equal(voxel.group_last(g), perm)
    a, b = voxel.group_last(g, seed=5), voxel.group_last(g, seed=5)
    assert torch.equal(a, b) and torch.equal(cluster[a], torch.arange(g.num_voxels))
    assert not torch.equal(a, voxel.group_last(g, seed=6))
    # a wide label range takes the relabelling route; ties go to the lowest label
    wide = torch.arange(cluster.numel()) % 1000
    h = R.histogram(wide, cluster, g.num_voxels, 1000)
    assert torch.equal(voxel.group_vote(wide, g), h.argmax(dim=-1))
    with pytest.raises(ValueError):
        voxel.group_histogram(f["y"], g, int(f["y"].max()))
    bad = f["pos"].clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        voxel.voxel_groups(bad, R.SIZE)
    far = torch.tensor([[-3000.0] * 3, [3000.0] * 3])
    with pytest.raises(ValueError, match="bits"):
        voxel.voxel_groups(far, 1e-3)
    # more points than an int32 index holds: refused on the host, before anything is allocated
    with pytest.raises(ValueError, match="points"):
        voxel.voxel_groups(torch.empty((2 ** 31, 3), device="meta"), R.FINE_SIZE)


def test_unsupported_keys_raise_like_the_reference(golden):
    from superpoint_transformer_amd.data import Cluster, Data
    from superpoint_transformer_amd.transforms import GridSampling3D
    pos = R.golden_fields(golden)["pos"][:50]
    with pytest.raises(NotImplementedError):
        GridSampling3D(R.SIZE)(Data(pos=pos, edge_index=torch.zeros(2, 3, dtype=torch.long)))
    with pytest.raises(NotImplementedError):
        GridSampling3D(R.SIZE)(Data(pos=pos, sub=torch.rand(50)))
    other = Cluster(torch.tensor([0, 50]), torch.arange(50))
    with pytest.raises(NotImplementedError):
        GridSampling3D(R.SIZE)(Data(pos=pos, parts=other))
    # inplace=False leaves the input alone; inplace=True returns it
    d = Data(pos=pos.clone(), tag="kept")
    out = GridSampling3D(R.SIZE)(d)
    assert out is not d and d.pos.shape[0] == 50 and out.tag == "kept"
    assert GridSampling3D(R.SIZE, inplace=True)(d) is d and d.pos.shape[0] < 50
    assert torch.equal(d.grid_size, torch.tensor([R.SIZE]))


def test_save_node_index_and_data_to():
    from superpoint_transformer_amd.data import Data
    from superpoint_transformer_amd.transforms import DataTo, SaveNodeIndex
    assert SaveNodeIndex.DEFAULT_KEY == "node_id"
    d = Data(pos=torch.rand(9, 3))
    assert SaveNodeIndex()(d) is d and torch.equal(d.node_id, torch.arange(9))
    assert d.node_id.dtype == torch.int64
    SaveNodeIndex(key="sub")(d)
    assert torch.equal(d.sub, torch.arange(9))
    t = DataTo("cpu")
    assert t.device == torch.device("cpu") and t(d) is d        # already there: the same object
    assert DataTo(torch.device("cpu")).device == torch.device("cpu")
