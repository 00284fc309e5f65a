"""CPU suite: tests/superedge_reference.py and the package's CPU route (``graph.subedges`` /
``graph.superedge_features`` / ``graph.minimalistic_edge_features`` / ``graph.connect_isolated`` on
CPU tensors) pinned on the fixtures the REFERENCE'S OWN functions produced
(tests/golden/superedges.npz, subedges.npz).  Criterion and bound: tests/test_superedges_gpu.py."""
import pytest
import torch

from conftest import load_golden, tl
import superedge_reference as R

GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))


@pytest.fixture(scope="module")
def g():
    return load_golden("superedges.npz")


def _level(g, lv):
    pos, si0, si1 = torch.from_numpy(g["pos"]), tl(g["super_index_0"]), tl(g["super_index_1"])
    _, _, _, ratio, se_min, cycles, margin = g[f"l{lv}_cfg"]
    kw = dict(ratio=float(ratio), k_min=int(se_min), cycles=int(cycles), margin=float(margin))
    ref = (tl(g[f"l{lv}_edge_index"]), tl(g[f"l{lv}_pairs"]), tl(g[f"l{lv}_uid"]))
    return pos, (si0 if lv == 1 else si1[si0]), tl(g[f"l{lv}_graph_edge_index"]), kw, ref


def _features_within_bound(g, lv, attr, same):
    bound = torch.from_numpy(g["bound"]).double()
    d = (attr.double() - torch.from_numpy(g[f"l{lv}_edge_attr"]).double()).abs()
    assert (d[:, GROUPS[0]] <= bound[0]).all()
    for k in (1, 2):
        assert (d[same][:, GROUPS[k]] <= bound[k]).all()


def test_fixture_has_what_the_tests_need(g):
    for lv in (1, 2):
        ei, n = tl(g[f"l{lv}_edge_index"]), int(g[f"pos_{lv}"].shape[0])
        assert (ei[0] < ei[1]).all()
        # the distant patch is the last node: it has exactly its k_min edges, from connect_isolated
        assert int((ei == n - 1).any(0).sum()) == int(g[f"l{lv}_cfg"][0])
        assert g[f"l{lv}_edge_attr"].shape == (ei.shape[1], 7)
    assert (g["bound"] > 0).all() and (g["bound"] < 1e-4).all()
    sizes = torch.bincount(tl(g["super_index_1"])[tl(g["super_index_0"])])
    assert int(sizes.max()) > 500                                # level 2: several hundred points


@pytest.mark.parametrize("lv", [1, 2])
def test_reference_restatement_on_the_fixture(g, lv):
    pos, index, ei, kw, ref = _level(g, lv)
    got_ei, pairs, uid, _ = R.subedges_reference(pos, index, ei, **kw)
    same, excused = R.compare_subedges((got_ei, pairs, uid), ref)
    assert not excused
    attr = R.edge_features_reference(pos, pairs, uid, got_ei.shape[1], dtype=torch.float32)
    _features_within_bound(g, lv, attr, same)
    f64 = R.edge_features_reference(pos, ref[1], ref[2], got_ei.shape[1])
    assert torch.allclose(f64, torch.from_numpy(g[f"l{lv}_edge_attr_f64"]), rtol=0, atol=1e-12)
    # the f64 restatement selects the same points: no key of this scene sits on a threshold
    e64, p64, u64, _ = R.subedges_reference(pos, index, ei, dtype=torch.float64, **kw)
    R.compare_subedges((e64, p64, u64), ref)


@pytest.mark.parametrize("lv", [1, 2])
def test_package_cpu_route_on_the_fixture(g, lv):
    from superpoint_transformer_amd import graph as G
    pos, index, ei, kw, ref = _level(g, lv)
    got_ei, attr, pairs, uid = G.superedge_features(pos, index, ei, return_pairs=True, **kw)
    same, _ = R.compare_subedges((got_ei, pairs, uid), ref)
    assert attr.dtype == torch.float32 and attr.shape == (got_ei.shape[1], 7)
    _features_within_bound(g, lv, attr, same)
    ei2, attr2 = G.superedge_features(pos, index, ei, **kw)
    assert torch.equal(ei2, got_ei) and torch.equal(attr2, attr)
    want = G.minimalistic_edge_features(pos.double(), ref[1], ref[2], got_ei.shape[1])
    assert torch.allclose(want, torch.from_numpy(g[f"l{lv}_edge_attr_f64"]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("c", [0, 1])
def test_package_cpu_subedges_on_the_subedges_fixture(c):
    from superpoint_transformer_amd import graph as G
    s = load_golden("subedges.npz")
    ratio, k_min, cycles, margin = s[f"c{c}_cfg"]
    kw = dict(ratio=float(ratio), k_min=int(k_min), cycles=int(cycles), margin=float(margin))
    pos, index, ei = torch.from_numpy(s["pos"]), tl(s["index"]), tl(s["edge_index"])
    ref = (tl(s[f"c{c}_edge_index"]), tl(s[f"c{c}_pairs"]), tl(s[f"c{c}_uid"]))
    R.compare_subedges(G.subedges(pos, index, ei, **kw), ref)
    R.compare_subedges(R.subedges_reference(pos, index, ei, **kw)[:3], ref)


@pytest.mark.parametrize("lv", [1, 2])
def test_connect_isolated_restores_the_patch_edges(g, lv):
    from superpoint_transformer_amd import graph as G
    ge = tl(g[f"l{lv}_graph_edge_index"])
    pos = torch.from_numpy(g[f"pos_{lv}"])
    n, k_min = pos.shape[0], int(g[f"l{lv}_cfg"][0])
    radius_only = ge[:, ~(ge == n - 1).any(0)]                  # what the radius search alone finds
    got = G.to_trimmed(G.connect_isolated(radius_only, pos, k_min, num_nodes=n))
    assert torch.equal(got, ge)
    assert G.connect_isolated(ge, pos, k_min) is ge              # nothing isolated: unchanged


def test_size_class_cloud_has_no_key_on_a_threshold():
    """The seeded cloud of the GPU size-class test: the f32 CPU route and the f64 restatement
    select the same points on every edge, so no edge of it should need the rounding excuse."""
    from superpoint_transformer_amd import graph as G
    from test_superedges_gpu import size_class_cloud
    pos, index, ei, _ = size_class_cloud(G.superedge_capacity())
    kw = dict(ratio=0.2, k_min=20, cycles=3, margin=0.2)
    got = G.subedges(pos, index, ei, **kw)
    want = R.subedges_reference(pos, index, ei, dtype=torch.float64, **kw)[:3]
    _, excused = R.compare_subedges(got, want)
    assert not excused


def test_transform_refusals_need_no_device():
    from superpoint_transformer_amd import transforms as T
    with pytest.raises(AssertionError):
        T.RadiusHorizontalGraph(k_min=0)
    with pytest.raises(AssertionError):
        T.RadiusHorizontalGraph(k_min=[2, 0])
    with pytest.raises(AssertionError):
        T.NAGRemoveKeys(level=1.5, keys=["x"])
    assert T.RadiusHorizontalGraph(keys="mean_off").keys == ("mean_off",)


def test_entries_refuse_on_the_host():
    """Argument checks run before any device access: 32-bit indices are a checked refusal."""
    from superpoint_transformer_amd import _lib, graph as G
    L = _lib.lib
    assert G.superedge_capacity() == L.spt_superedge_capacity() >= 128
    assert L.spt_superedge_workspace_bytes(1000) > 3 * 4 * 1001
    args = [None, 0, None, None, 4, None, 2, 2, None, None, 1, 1, 0.2, 20, 0.2, 7, 0, None, None, None,
            None, None, 0, None]
    too_many = list(args)
    too_many[1] = 2 ** 31
    assert L.spt_superedge_f32(*too_many) != 0 and "2^31 - 1 points" in _lib.last_error()
    assert L.spt_superedge_f32(*args) != 0 and "null pointer" in _lib.last_error()
    classes = list(args)
    classes[10] = 2
    assert L.spt_superedge_f32(*classes) != 0 and "class counts" in _lib.last_error()
    assert L.spt_superedge_classify(None, 4, None, 2, 2, None, None, None, 0, None) != 0
    assert L.spt_superedge_pair_offsets(None, 5, None, None, 0, None) != 0
    pos = torch.zeros(4, 2)
    with pytest.raises(Exception):
        G.minimalistic_edge_features(pos, torch.zeros(2, 3), torch.zeros(3), 1)
