"""``graph.superedge_features`` on ``csrc/superedge.hip`` - subedges and the 7 stored edge features
in one pass per edge - and the transforms built on it.

References: the fixtures the REFERENCE'S OWN functions produced (tests/golden/subedges.npz,
superedges.npz), the ``graph.subedges`` composition on the same device, and the plain-torch
restatement tests/superedge_reference.py.  What "equal" means for subedges is
``superedge_reference.compare_subedges`` (tests/test_subedges.py's criterion): edge list, uid and
count exact, the selected point sets of every edge exact, the pairing up to the target-side
reversal that the sign of an eigenvector leaves open, on at most a third of the edges.

Features: ``mean_off`` does not depend on the pairing and is compared on every edge; ``std_off``
and ``mean_dist`` are compared with the reference's output where the pairing is the fixture's, and
on every edge with the f64 closed form evaluated on the kernel's own pairs.  The bound is read from
the fixture: 4 x the deviation of the reference's own f32 output from its f64 evaluation, per
column group (profiles/r21a_superedge_errors.txt), measured on coordinates of extent 30; every
synthetic cloud here stays within that extent.
"""
import pytest
import torch

from conftest import load_golden, tl
import superedge_reference as R

pytestmark = pytest.mark.gpu

GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))
EXTENT = 30.0


def _bound():
    return torch.from_numpy(load_golden("superedges.npz")["bound"]).double()


def _run(dev, pos, index, edge_index, **kw):
    from superpoint_transformer_amd import graph as G
    ei, attr, pairs, uid = G.superedge_features(pos.to(dev), index.to(dev), edge_index.to(dev),
                                                return_pairs=True, **kw)
    ei2, attr2 = G.superedge_features(pos.to(dev), index.to(dev), edge_index.to(dev), **kw)
    assert torch.equal(ei, ei2) and torch.equal(attr, attr2)       # the route without pairs
    assert attr.dtype == torch.float32 and attr.shape == (ei.shape[1], 7)
    assert pairs.dtype == torch.int64 and uid.dtype == torch.int64
    return ei.cpu(), attr.cpu(), pairs.cpu(), uid.cpu()


def _check_features(attr, pos, pairs, uid, ref_attr=None, same=None, skip=()):
    """attr against the f64 closed form on its own pairs (all edges), and against the
    reference's output: mean_off everywhere, the rest where the pairing is the reference's."""
    bound = _bound()
    E = attr.shape[0]
    keep = torch.ones(E, dtype=torch.bool)
    keep[list(skip)] = False
    own = R.edge_features_reference(pos, pairs, uid, E)
    assert torch.isfinite(attr).all()
    for g, cols in enumerate(GROUPS):
        d = (attr.double() - own)[keep][:, cols].abs()
        print(f"group {g}: |kernel - f64 closed form| max {float(d.max()) if d.numel() else 0:.3e} "
              f"bound {float(bound[g]):.3e}")
        assert (d <= bound[g]).all()
    if ref_attr is not None:
        d = (attr.double() - ref_attr.double()).abs()
        print(f"|kernel - reference| mean_off max {float(d[keep][:, GROUPS[0]].max()):.3e}")
        assert (d[keep][:, GROUPS[0]] <= bound[0]).all()
        for g in (1, 2):
            assert (d[same & keep][:, GROUPS[g]] <= bound[g]).all()


def _cfg_sub(g, c):
    ratio, k_min, cycles, margin = g[f"c{c}_cfg"]
    return dict(ratio=float(ratio), k_min=int(k_min), cycles=int(cycles), margin=float(margin))


def _cfg_level(g, lv):
    _, _, _, ratio, se_min, cycles, margin = g[f"l{lv}_cfg"]
    return dict(ratio=float(ratio), k_min=int(se_min), cycles=int(cycles), margin=float(margin))


# ---- fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 1])
def test_subedges_fixture(c, dev):
    g = load_golden("subedges.npz")
    pos = torch.from_numpy(g["pos"])
    ei, attr, pairs, uid = _run(dev, pos, tl(g["index"]), tl(g["edge_index"]), **_cfg_sub(g, c))
    R.compare_subedges((ei, pairs, uid),
                       (tl(g[f"c{c}_edge_index"]), tl(g[f"c{c}_pairs"]), tl(g[f"c{c}_uid"])))
    _check_features(attr, pos, pairs, uid)


@pytest.mark.parametrize("lv", [1, 2])
def test_superedges_fixture(lv, dev):
    g = load_golden("superedges.npz")
    pos, si0, si1 = torch.from_numpy(g["pos"]), tl(g["super_index_0"]), tl(g["super_index_1"])
    index = si0 if lv == 1 else si1[si0]
    ei, attr, pairs, uid = _run(dev, pos, index, tl(g[f"l{lv}_graph_edge_index"]), **_cfg_level(g, lv))
    same, _ = R.compare_subedges((ei, pairs, uid), (tl(g[f"l{lv}_edge_index"]), tl(g[f"l{lv}_pairs"]),
                                                    tl(g[f"l{lv}_uid"])))
    _check_features(attr, pos, pairs, uid, torch.from_numpy(g[f"l{lv}_edge_attr"]), same)


# ---- size classes -----------------------------------------------------------------------------
def size_class_cloud(C, seed=20241):
    """Two segments each of 1, 2, 63, 64, 65, C - 1, C and C + 1 points: blobs of radius ~1 on a
    ring of radius 6, every segment joined with every other."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [1, 2, 63, 64, 65, C - 1, C, C + 1] * 2
    pts, idx = [], []
    for s, n in enumerate(sizes):
        a = torch.tensor(6.283185 * ((s * 7) % len(sizes)) / len(sizes))
        centre = torch.stack((6 * torch.cos(a), 6 * torch.sin(a), torch.tensor(0.3 * s)))
        pts.append(centre + (torch.rand(n, 3, generator=gen) - 0.5) * torch.tensor([3.0, 3.0, 1.0]))
        idx.append(torch.full((n,), s))
    pos, index = torch.cat(pts).float(), torch.cat(idx)
    perm = torch.randperm(pos.shape[0], generator=gen)
    S = len(sizes)
    ei = torch.triu(torch.ones(S, S), diagonal=1).nonzero().t().contiguous()
    return pos[perm], index[perm], ei, sizes


def test_size_classes_against_composition(dev):
    from superpoint_transformer_amd import graph as G
    C = G.superedge_capacity()
    assert C >= 128
    pos, index, ei, sizes = size_class_cloud(C)
    kw = dict(ratio=0.2, k_min=20, cycles=3, margin=0.2)
    got_ei, attr, pairs, uid = _run(dev, pos, index, ei, **kw)
    ref = tuple(t.cpu() for t in G.subedges(pos.to(dev), index.to(dev), ei.to(dev), **kw))
    anchors = R.pair_anchors(pos, index, R.to_trimmed(ei), kw["cycles"], len(sizes))
    L = float((pos.max(0).values - pos.min(0).values).max())
    tol = 8 * 2.0 ** -23 * L

    def allow(e, s, t, rs, rt):
        near = R.edge_thresholds(pos, index, int(got_ei[0, e]), int(got_ei[1, e]), int(anchors[0, e]),
                                 int(anchors[1, e]), kw["ratio"], kw["k_min"], kw["margin"])
        differing = (set(s) ^ set(rs)) | (set(t) ^ set(rt))
        return all(near[q] <= tol for q in differing)

    same, excused = R.compare_subedges((got_ei, pairs, uid), ref, allow=allow)
    E = got_ei.shape[1]
    assert E == len(sizes) * (len(sizes) - 1) // 2
    assert len(excused) <= E // 100, f"{len(excused)} of {E} edges needed the rounding excuse"
    ref_attr = G.minimalistic_edge_features(pos.to(dev), ref[1].to(dev), ref[2].to(dev), E).cpu()
    _check_features(attr, pos, pairs, uid, ref_attr, same, skip=excused)
    # every route was taken
    big = torch.tensor(sizes)[got_ei].max(0).values
    assert (big <= 64).any() and ((big > 64) & (big <= C)).any() and (big > C).any()


# ---- degenerate edges and the switches --------------------------------------------------------
def _blobs(gen, sizes, spread=1.0, step=1.2):
    pts = [torch.rand(n, 3, generator=gen) * spread + torch.tensor([step * s, 0.0, 0.0])
           for s, n in enumerate(sizes)]
    idx = [torch.full((n,), s) for s, n in enumerate(sizes)]
    return torch.cat(pts).float(), torch.cat(idx)


def _chain(n):
    return torch.stack((torch.arange(n - 1), torch.arange(1, n)))


def _degenerate_cases():
    gen = torch.Generator().manual_seed(99)
    cases = {}
    pos, idx = _blobs(gen, [40, 50, 30])
    pos[0] = pos[40] = torch.tensor([1.1, 0.5, 0.5])                    # segments 0 and 1 share a point
    idx[0], idx[40] = 0, 1
    cases["same_anchor"] = (pos, idx, _chain(3), {}, True)
    a = torch.cat((torch.zeros(1, 3), torch.rand(30, 3, generator=gen) - 2.5))
    b = torch.cat((torch.full((1, 3), 0.5), torch.rand(45, 3, generator=gen) + 2.0))
    cases["diagonal"] = (torch.cat((a, b)).float(), torch.cat((torch.zeros(31), torch.ones(46))).long(),
                         _chain(2), {}, True)
    x = torch.cat((torch.rand(25, generator=gen), 1.2 + torch.rand(70, generator=gen)))
    cases["collinear"] = (torch.stack((x, torch.zeros(95), torch.zeros(95)), 1).float(),
                          torch.cat((torch.zeros(25), torch.ones(70))).long(), _chain(2), {}, True)
    cases["coincident"] = (torch.cat((torch.zeros(12, 3), torch.ones(9, 3))).float(),
                           torch.cat((torch.zeros(12), torch.ones(9))).long(), _chain(2),
                           dict(k_min=4), False)
    pos, idx = _blobs(gen, [30, 80, 200, 7])
    cases["emptying_filter"] = (pos, idx, _chain(4), dict(margin=-5.0), True)
    cases["k_min_above_size"] = (pos, idx, _chain(4), dict(k_min=1000), True)
    cases["ratio_one"] = (pos, idx, _chain(4), dict(ratio=1.0, k_min=1), True)
    for name in ("halfspace_filter", "bbox_filter", "target_pc_flip"):
        cases[f"no_{name}"] = (pos, idx, _chain(4), {name: False}, True)
    cases["no_filters"] = (pos, idx, _chain(4), dict(halfspace_filter=False, bbox_filter=False), True)
    cases["source_pc_sort"] = (pos, idx, _chain(4), dict(source_pc_sort=True), True)
    cases["source_pc_sort_no_flip"] = (pos, idx, _chain(4), dict(source_pc_sort=True,
                                                                target_pc_flip=False), True)
    return cases


CASES = _degenerate_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_degenerate_edges_and_switches(name, dev):
    pos, index, ei, kw, pairing = CASES[name]
    got_ei, attr, pairs, uid = _run(dev, pos, index, ei, **kw)
    r_ei, r_pairs, r_uid, _ = R.subedges_reference(pos, index, ei, **kw)
    if pairing:
        R.compare_subedges((got_ei, pairs, uid), (r_ei, r_pairs, r_uid))
    else:                                       # zero covariance: any direction is a first component
        assert torch.equal(got_ei, r_ei) and torch.equal(uid, r_uid)
        for (s, t), (rs, rt) in zip(R.per_edge(pairs, uid, ei.shape[1]), R.per_edge(r_pairs, r_uid, ei.shape[1])):
            assert sorted(s) == sorted(rs) and sorted(t) == sorted(rt)
    _check_features(attr, pos, pairs, uid)
    cnt = torch.bincount(uid, minlength=got_ei.shape[1])
    assert (cnt >= 1).all()
    if name == "k_min_above_size":
        size = torch.bincount(index)
        assert (cnt <= torch.minimum(size[got_ei[0]], size[got_ei[1]])).all()


def test_no_edges(dev):
    from superpoint_transformer_amd import graph as G
    pos, idx = torch.rand(50, 3).to(dev), (torch.arange(50) // 10).to(dev)
    for e in (torch.empty((2, 0), dtype=torch.long), torch.tensor([[1, 2], [1, 2]])):   # loops vanish
        ei, attr, pairs, uid = G.superedge_features(pos, idx, e.to(dev), return_pairs=True)
        assert ei.shape == (2, 0) and attr.shape == (0, 7) and pairs.shape == (2, 0) and uid.numel() == 0


def test_refuses_cpu_mix_and_bad_shapes(dev):
    from superpoint_transformer_amd import graph as G
    pos, idx = torch.rand(50, 3).to(dev), (torch.arange(50) // 10).to(dev)
    with pytest.raises(RuntimeError):
        G.superedge_features(pos, idx.cpu(), torch.tensor([[0], [1]]).to(dev))
    with pytest.raises(ValueError):
        G.superedge_features(pos[:, :2], idx, torch.tensor([[0], [1]]).to(dev))


# ---- reproducibility --------------------------------------------------------------------------
def test_two_runs_are_bit_equal(dev):
    from superpoint_transformer_amd import graph as G
    pos, index, ei, _ = size_class_cloud(G.superedge_capacity(), seed=5)
    a = _run(dev, pos, index, ei)
    b = _run(dev, pos, index, ei)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- memory contract --------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
def test_entries_between_guards(poison, dev):
    """The C entries themselves: every input flush against a guard, every output and the scratch
    cut to the byte, once more with outputs and scratch NaN-filled; results equal the wrapper's."""
    from guarded import GuardedArena
    from superpoint_transformer_amd import _lib, graph as G
    from superpoint_transformer_amd.csr import csr_of
    from superpoint_transformer_amd.neighbors import _pair_anchors
    L = _lib.lib
    C = G.superedge_capacity()
    pos, index, ei, _ = size_class_cloud(C, seed=11)
    keep = torch.bincount(index)[ei].max(0).values <= C            # the kernel's own edges
    ei = G.to_trimmed(ei[:, keep])
    kw = dict(ratio=0.3, k_min=7, cycles=2, margin=0.15)
    want = _run(dev, pos, index, ei, **kw)
    E, N = ei.shape[1], pos.shape[0]

    arena = GuardedArena(dev, guard_byte=0xFF if poison else 0xA5, fill_byte=0xFF if poison else None)
    posd, indexd = pos.to(dev), index.to(dev)
    csr = csr_of(indexd, int(index.max()) + 1)
    anchors, _ = _pair_anchors(posd, indexd, ei.to(dev), kw["cycles"], csr.num_seg)
    p = arena.place(posd, label="pos")
    rowptr = arena.place(csr.rowptr, guard_byte=0x00, label="rowptr")
    perm = arena.place(csr.perm, guard_byte=0x00, label="perm")
    edges = arena.place(ei.to(dev), guard_byte=0x00, label="edge_index")
    anc = arena.place(anchors, guard_byte=0x00, label="anchors")
    nbytes = L.spt_superedge_workspace_bytes(E)
    order = arena.take(4 * E, torch.int32, (E,), "order")
    counts = arena.take(24, torch.int64, (3,), "counts")
    attr = arena.take(28 * E, torch.float32, (E, 7), "edge_attr")
    count = arena.take(4 * E, torch.int32, (E,), "count")
    offsets = arena.take(4 * (E + 1), torch.int32, (E + 1,), "offsets")
    stream = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        ws = arena.take(nbytes, label="classify ws")
        _lib.check(L.spt_superedge_classify(rowptr.data_ptr(), csr.num_seg, edges.data_ptr(), E, E,
                                            order.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
                                            stream), "classify")
        n_small, n_medium, n_large = counts.tolist()
        assert n_large == 0 and n_small > 0 and n_medium > 0

        def launch(count_only, off, pairs, uid, M):
            _lib.check(L.spt_superedge_f32(
                p.data_ptr(), N, perm.data_ptr(), rowptr.data_ptr(), csr.num_seg, edges.data_ptr(), E, E,
                anc.data_ptr(), order.data_ptr(), n_small, n_medium, kw["ratio"], kw["k_min"],
                kw["margin"], 7, count_only, attr.data_ptr(), count.data_ptr(), off,
                pairs, uid, M, stream), "superedge")
        launch(1, None, None, None, 0)
        M = int(count.sum())
        ws = arena.take(nbytes, label="offsets ws")
        _lib.check(L.spt_superedge_pair_offsets(count.data_ptr(), E, offsets.data_ptr(), ws.data_ptr(),
                                                nbytes, stream), "offsets")
        pairs = arena.take(16 * M, torch.int64, (2, M), "pairs")
        uid = arena.take(8 * M, torch.int64, (M,), "uid")
        launch(0, offsets.data_ptr(), pairs.data_ptr(), uid.data_ptr(), M)
    arena.check()
    assert int(offsets[E]) == M
    assert torch.equal(attr.cpu(), want[1]) and torch.equal(pairs.cpu(), want[2])
    assert torch.equal(uid.cpu(), want[3])
    assert torch.equal(count.cpu().long(), torch.bincount(want[3], minlength=E))


def test_wrapper_under_exact_workspaces(dev):
    from guarded import GuardedArena, exact_workspaces, poisoned_fresh_tensors
    from superpoint_transformer_amd import graph as G
    pos, index, ei, _ = size_class_cloud(G.superedge_capacity(), seed=13)
    want = _run(dev, pos, index, ei)
    arena = GuardedArena(dev, guard_byte=0xFF, fill_byte=0xFF)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        got = _run(dev, pos, index, ei)
    for x, y in zip(want, got):
        assert torch.equal(x, y)


# ---- wrapper ----------------------------------------------------------------------------------
def test_wrapper_layouts(dev):
    from superpoint_transformer_amd import graph as G
    g = load_golden("superedges.npz")
    pos, index = torch.from_numpy(g["pos"]).to(dev), tl(g["super_index_0"]).to(dev)
    ei = tl(g["l1_graph_edge_index"]).to(dev)
    kw = _cfg_level(g, 1)
    want = G.superedge_features(pos, index, ei, return_pairs=True, **kw)
    table = torch.randn(pos.shape[0], 7, device=dev)
    table[:, 2:5] = pos
    wide = torch.cat((torch.full((2, 3), 5, device=dev), ei), dim=1)
    for p, i, e in ((table[:, 2:5], index, ei), (pos, index, wide[:, 3:]),
                    (pos, index.int(), ei.int()), (table[:, 2:5], index.int(), wide[:, 3:].int())):
        assert e.shape == ei.shape
        got = G.superedge_features(p, i, e, return_pairs=True, **kw)
        for x, y in zip(want, got):
            assert torch.equal(x, y)


# ---- transforms -------------------------------------------------------------------------------
def _fixture_nag(dev):
    from superpoint_transformer_amd.data import Data, NAG
    g = load_golden("superedges.npz")
    pos, si0, si1 = torch.from_numpy(g["pos"]), tl(g["super_index_0"]), tl(g["super_index_1"])
    nag = NAG([Data(pos=pos.to(dev), super_index=si0.to(dev)),
               Data(pos=torch.from_numpy(g["pos_1"]).to(dev), super_index=si1.to(dev)),
               Data(pos=torch.from_numpy(g["pos_2"]).to(dev))])
    return g, nag


def _level_lists(g):
    cfg = {lv: g[f"l{lv}_cfg"] for lv in (1, 2)}
    col = lambda j, cast: [cast(cfg[1][j]), cast(cfg[2][j])]       # noqa: E731
    return dict(k_min=col(0, int), k_max=col(1, int), gap=col(2, float), se_ratio=col(3, float),
                se_min=col(4, int), cycles=col(5, int), margin=col(6, float))


def test_radius_horizontal_graph_on_the_fixture(dev):
    from superpoint_transformer_amd import transforms as T
    g, nag = _fixture_nag(dev)
    nag = T.RadiusHorizontalGraph(pca_on_cpu=True, chunk_size=7, verbose=False, **_level_lists(g))(nag)
    for lv in (1, 2):
        ref_ei = tl(g[f"l{lv}_edge_index"])
        ei, attr = nag[lv].edge_index.cpu(), nag[lv].edge_attr.cpu()
        assert torch.equal(ei, ref_ei)                              # the patch's k_min edges included
        last = nag[lv].num_nodes - 1
        assert int((ei == last).any(0).sum()) == int(g[f"l{lv}_cfg"][0])
        ref_attr = torch.from_numpy(g[f"l{lv}_edge_attr"])
        bound = _bound()
        assert ((attr.double() - ref_attr.double())[:, GROUPS[0]].abs() <= bound[0]).all()
        # the rest of the columns through the kernel's own pairs: the same call with pairs
        from superpoint_transformer_amd import graph as G
        _, attr2, pairs, uid = G.superedge_features(
            nag[0].pos, nag.get_super_index(lv), nag[lv].edge_index, return_pairs=True,
            num_segments=nag[lv].num_nodes, **_cfg_level(g, lv))
        assert torch.equal(attr2.cpu(), attr)
        same, _ = R.compare_subedges((ei, pairs, uid), (ref_ei, tl(g[f"l{lv}_pairs"]), tl(g[f"l{lv}_uid"])))
        _check_features(attr, torch.from_numpy(g["pos"]), pairs, uid, ref_attr, same)


def test_radius_horizontal_graph_scalar_parameters_and_refusals(dev):
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.data import Data, NAG
    g, nag = _fixture_nag(dev)
    lists = _level_lists(g)
    scalars = {k: v[0] for k, v in lists.items()}
    a = T.RadiusHorizontalGraph(**scalars)(nag.clone())
    b = T.RadiusHorizontalGraph(**{k: [v, v] for k, v in scalars.items()})(nag.clone())
    for lv in (1, 2):
        assert torch.equal(a[lv].edge_index, b[lv].edge_index)
        assert torch.equal(a[lv].edge_attr, b[lv].edge_attr)
    assert torch.equal(a[1].edge_index.cpu(), tl(g["l1_edge_index"]))
    with pytest.raises(AssertionError):
        T.RadiusHorizontalGraph(k_min=0)
    with pytest.raises(AssertionError):
        T.RadiusHorizontalGraph(k_min=[1, 0])
    with pytest.raises(NotImplementedError):
        T.RadiusHorizontalGraph(keys=["mean_off", "std_off"])(nag.clone())
    one = NAG([nag[0].clone(), Data(pos=torch.zeros(1, 3, device=dev))])
    one[0].super_index = torch.zeros_like(one[0].super_index)
    with pytest.raises(ValueError):
        T.RadiusHorizontalGraph()(one)


def test_segment_features_and_on_the_fly_features(dev):
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.segment import SEGMENT_BASE_FEATURES, segment_features
    g, nag = _fixture_nag(dev)
    gen = torch.Generator().manual_seed(3)
    nag[0].intensity = torch.rand(nag[0].num_nodes, 1, generator=gen).to(dev)
    nag[0].normal = torch.nn.functional.normalize(torch.randn(nag[0].num_nodes, 3, generator=gen)).to(dev)
    tr = T.SegmentFeatures(n_max=32, n_min=5, mean_keys=["intensity", "normal"], std_keys=["intensity"])
    torch.manual_seed(77)
    out = tr(nag.clone())
    torch.manual_seed(77)
    attrs = {"intensity": nag[0].intensity, "normal": nag[0].normal}
    for lv in (1, 2):
        want = segment_features(nag[0].pos, nag.get_super_index(lv), nag[lv].num_nodes,
                                n_max=32, n_min=5, mean_keys=["intensity", "normal"],
                                std_keys=["intensity"], point_attrs=attrs)
        names = set(SEGMENT_BASE_FEATURES) | {"mean_intensity", "mean_normal", "std_intensity"}
        assert set(want) == names
        for k in names:
            assert torch.equal(out[lv][k], want[k]), k
    with pytest.raises(ValueError):
        T.SegmentFeatures(mean_keys=["rgb"], std_keys=[])(nag.clone())
    loose = T.SegmentFeatures(mean_keys=["rgb"], std_keys=[], strict=False)(nag.clone())
    assert "mean_rgb" not in loose[1] and "log_size" in loose[1]
    # the chain's last steps: the stored 7 features feed the on-the-fly 18
    out = T.RadiusHorizontalGraph(**_level_lists(g))(out)
    E = out[1].edge_index.shape[1]
    assert out[1].edge_attr.shape == (E, 7) and out[1].edge_attr.dtype == torch.float32
    out = T.NAGRemoveKeys(level="1+", keys=["std_intensity"])(out)
    assert "std_intensity" not in out[1] and "mean_intensity" in out[1]
    with pytest.raises(Exception):
        T.NAGRemoveKeys(level=1, keys=["nothing"], strict=True)(out)
    out = T.OnTheFlyHorizontalEdgeFeatures(add_self_loops=False)(out)
    assert out[1].edge_attr.shape == (2 * E, len(T.EDGE_FEATURE_COLUMNS))
    assert out[1].edge_attr.dtype == torch.float32 and torch.isfinite(out[1].edge_attr).all()
