"""The kernels of csrc/predict.hip against the reference-made fixture
(tests/golden/semantic_output.npz) and, at the shapes where they can go wrong, against torch on
the CPU.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

C = 13
KEY = "tta_node_id"


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in load_golden("semantic_output.npz").items()}


def bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


def cluster_of(ptr, pts, dev):
    from superpoint_transformer_amd.data import Cluster
    return Cluster(ptr.to(dev), pts.to(dev))


# ---- row_argmax ----------------------------------------------------------------------------------
def awkward_logits(rows, c, seed):
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(rows, c, generator=gen) * 2).round() / 2          # many exact ties
    r = torch.arange(rows)
    z[r % 7 == 3] = 0.25                                                # all equal
    z[r % 11 == 5] = float("-inf")
    z[r % 13 == 6, c // 2] = float("nan")
    two = r % 17 == 9
    z[two, 0] = float("nan")
    z[two, c - 1] = float("nan")
    z[r % 19 == 4, c - 1] = float("inf")
    return z


@pytest.mark.parametrize("c", [1, 2, 13, 20, 32, 33, 70])
def test_row_argmax_matches_torch(c, dev):
    from superpoint_transformer_amd import predict
    for rows in (1, 63, 64, 65, 1000):
        z = awkward_logits(rows, c, 100 * c + rows)
        got = predict.row_argmax(z.to(dev))
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.argmax(z, dim=1)), (rows, c)


def test_void_mask_matches_torch_true_division(dev):
    from superpoint_transformer_amd import predict
    gen = torch.Generator().manual_seed(5)
    for rows, ncols in ((1, 1), (65, 14), (1000, 14), (257, 2)):
        h = torch.randint(0, 30, (rows, ncols), generator=gen)
        h[::5, -1] = h[::5, :-1].sum(dim=1)                              # exactly half
        h[1::5, -1] = h[1::5, :-1].sum(dim=1) + 1                        # one over
        h[2::5] = 0                                                      # 0 / 0
        big = torch.randint(1 << 24, 1 << 40, (rows,), generator=gen)
        h[3::5, 0] = big[3::5]
        h[3::5, -1] = big[3::5] + torch.randint(0, 3, (rows,), generator=gen)[3::5]
        want = h[:, -1] / h.sum(dim=1) > 0.5
        assert torch.equal(predict.void_mask(h.to(dev)).cpu(), want), (rows, ncols)
        z = awkward_logits(rows, 13, rows)
        pred, void = predict.row_argmax(z.to(dev), h.to(dev))
        assert torch.equal(pred.cpu(), torch.argmax(z, dim=1)) and torch.equal(void.cpu(), want)


# ---- the fixture through the kernels -------------------------------------------------------------
def test_fixture_predictions_hops_and_matrices(g, dev):
    from superpoint_transformer_amd import predict
    from superpoint_transformer_amd.output import SemanticSegmentationOutput
    d = {k: v.to(dev) for k, v in g.items()}
    si01, si_raw0 = d["in__si01"], d["in__si_raw0"]
    sub1 = cluster_of(g["in__sub1_pointers"], g["in__sub1_points"], dev)     # 120 voxels, empties
    sub0 = cluster_of(g["in__sub0_pointers"], g["in__sub0_points"], dev)     # 2 x 200 points, empties
    outs = {"single": SemanticSegmentationOutput(d["in__logits_single"], d["in__y_hist"]),
            "multi": SemanticSegmentationOutput([d["in__logits_multi1"], d["in__logits_multi2"]],
                                                [d["in__y_hist"], d["in__y_hist"][:9]])}
    for name, o in outs.items():
        assert o.device.type == "cuda"
        assert torch.equal(o.semantic_pred().cpu(), g[f"{name}__semantic_pred"])
        assert torch.equal(o.void_mask.cpu(), g[f"{name}__void_mask"])
        for kw in (dict(super_index=si01), dict(sub=sub1)):
            assert torch.equal(o.voxel_semantic_pred(**kw).cpu(), g[f"{name}__voxel_semantic_pred"])
            assert torch.equal(o.confusion_matrix(C, d["in__y_voxel"], "voxel", **kw).cpu(),
                               g[f"{name}__confmat_voxel"])
        for kw in (dict(super_index_level0_to_level1=si01, super_index_raw_to_level0=si_raw0),
                   dict(sub_level1_to_level0=sub1, sub_level0_to_raw=sub0),
                   dict(super_index_level0_to_level1=si01, sub_level0_to_raw=sub0),
                   dict(sub_level1_to_level0=sub1, super_index_raw_to_level0=si_raw0)):
            assert torch.equal(o.full_res_semantic_pred(**kw).cpu(),
                               g[f"{name}__full_res_semantic_pred"]), sorted(kw)
            assert torch.equal(o.confusion_matrix(C, d["in__y_raw"], "raw", **kw).cpu(),
                               g[f"{name}__confmat_raw"]), sorted(kw)
        both = predict.labels_through(o.semantic_pred(), [sub1, sub0])
        assert torch.equal(both["voxel"].cpu(), g[f"{name}__voxel_semantic_pred"])


@pytest.mark.parametrize("case,levels", [("single", 1), ("multi", 2)])
def test_fixture_multi_run(g, case, levels, dev):
    from superpoint_transformer_amd.data import NAG, Data
    from superpoint_transformer_amd.output import MultiRunInference, SemanticSegmentationOutput
    lv1 = Data(pos=g[f"{case}__in__pos"].to(dev))
    if f"{case}__in__batch" in g:
        lv1.batch = g[f"{case}__in__batch"].to(dev)
    nag = NAG([Data(pos=torch.zeros(257, 3, device=dev)), lv1, Data(pos=torch.zeros(9, 3, device=dev))])
    mri = MultiRunInference(C, multi_stage=levels == 2, key=KEY, r_max=2)
    om = mri.empty_output(nag)
    for r in range(3):
        z = [g[f"{case}__in__run{r}_logits{lv}"].to(dev) for lv in range(1, levels + 1)]
        ids = [None] + [{KEY: g[f"{case}__in__run{r}_node_id{lv}"].to(dev)} for lv in range(1, levels + 1)]
        mri.update(om, SemanticSegmentationOutput(z if levels == 2 else z[0]), ids)
        acc = om.logits if levels == 2 else [om.logits]
        for lv in range(levels):
            assert bits(acc[lv], g[f"{case}__acc_run{r}_level{lv + 1}"]), (r, lv)
    assert torch.equal(mri.seen(om).cpu(), g[f"{case}__seen"])
    mri.finalize(om, nag)                                   # the device's own knn_2
    fin = om.logits if levels == 2 else [om.logits]
    for lv in range(levels):
        assert bits(fin[lv], g[f"{case}__final_level{lv + 1}"]), lv


# ---- accumulate_rows_ ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 300])
def test_accumulate_rows_bitwise_and_stamp(n, dev):
    from superpoint_transformer_amd import predict
    N = 300
    gen = torch.Generator().manual_seed(n)
    ref = torch.randn(N, C, generator=gen)
    acc = ref.to(dev)
    stamp = torch.zeros(N, dtype=torch.int32, device=dev)
    want_stamp = torch.zeros(N, dtype=torch.int32)
    for run in (1, 2, 3):
        ids = torch.randperm(N, generator=gen)[:n]
        src = torch.randn(n, C, generator=gen) * 10.0 ** (run - 2)
        ref[ids] += src                                      # the reference's index_put
        want_stamp[ids] = run
        res = predict.accumulate_rows_(acc, src.to(dev), ids.to(dev), stamp, run)
        assert res is acc and bits(acc, ref), run
        assert torch.equal(stamp.cpu(), want_stamp), run


def test_accumulate_rows_reports_duplicates_and_range(dev):
    from superpoint_transformer_amd import predict
    N = 300
    gen = torch.Generator().manual_seed(9)
    base = torch.randn(N, C, generator=gen)
    src = torch.randn(65, C, generator=gen)
    ids = torch.randperm(N, generator=gen)[:65]
    ids[40] = ids[3]                                         # a duplicate
    ids[50] = N                                              # one past the end
    ids[51] = -1
    for check in (True, False):
        acc = base.to(dev)
        stamp = torch.zeros(N, dtype=torch.int32, device=dev)
        if check:
            with pytest.raises(ValueError, match=r"1 node id.s. occur more than once in run 1; "
                                                 r"2 node id.s. lie outside \[0, 300\)"):
                predict.accumulate_rows_(acc, src.to(dev), ids.to(dev), stamp, 1)
        else:
            predict.accumulate_rows_(acc, src.to(dev), ids.to(dev), stamp, 1, check=False)
        got = acc.cpu()
        ok = torch.ones(65, dtype=torch.bool)
        ok[[3, 40, 50, 51]] = False
        want = base.clone()
        want[ids[ok]] += src[ok]
        twice = int(ids[3])
        rest = torch.ones(N, dtype=torch.bool)
        rest[twice] = False
        assert bits(got[rest], want[rest])                   # nothing written that should not be
        assert bits(got[twice], base[twice] + src[3]) or bits(got[twice], base[twice] + src[40])
        want_stamp = torch.zeros(N, dtype=torch.int32)
        want_stamp[ids[ok]] = 1
        want_stamp[twice] = 1
        assert torch.equal(stamp.cpu(), want_stamp)


# ---- labels_through ------------------------------------------------------------------------------
def hierarchy(n_raw, seed, sparse=False):
    """(label, si01, si_raw0, (ptr1, pts1), (ptr0, pts0)): a random three-level hierarchy over
    ``n_raw`` raw points with skewed sizes, empty clusters and shuffled Cluster points.
    ``sparse``: thousands of empty voxels, more pointers per tile than the kernel stages."""
    rng = np.random.default_rng(seed)
    n_vox = 5000 if sparse else max(1, n_raw // 4)
    n_sp = max(1, n_vox // 8)

    def hop(n_fine, n_coarse, allowed):
        w = rng.random(len(allowed)) ** 4                     # a few large clusters among small ones
        si = np.sort(rng.choice(allowed, n_fine, p=w / w.sum()))
        si = si[rng.permutation(n_fine)]
        sizes = np.bincount(si, minlength=n_coarse)
        ptr = np.concatenate(([0], np.cumsum(sizes)))
        pts = np.argsort(si, kind="stable")
        for a, b in zip(ptr[:-1], ptr[1:]):
            pts[a:b] = pts[a:b][rng.permutation(b - a)]
        return torch.from_numpy(si), (torch.from_numpy(ptr), torch.from_numpy(pts))

    sp_allowed = np.arange(n_sp)[1:-1] if n_sp > 3 else np.arange(n_sp)   # empties at both ends
    vox_allowed = rng.choice(n_vox, min(n_vox, max(1, n_raw // 3)), replace=False) if sparse \
        else (np.arange(n_vox)[1:-1] if n_vox > 3 else np.arange(n_vox))
    si01, sub1 = hop(n_vox, n_sp, sp_allowed)
    si_raw0, sub0 = hop(n_raw, n_vox, np.sort(vox_allowed))
    label = torch.from_numpy(rng.integers(0, 34, n_sp))
    return label, si01, si_raw0, sub1, sub0


def materialised(label, si01, si_raw0):
    return label[si01], label[si01][si_raw0]


@pytest.mark.parametrize("n_raw,sparse", [(1, False), (255, False), (256, False), (257, False),
                                          (1025, False), (4100, False), (3000, True)])
def test_labels_through_every_hop_combination(n_raw, sparse, dev):
    from superpoint_transformer_amd import ops, predict
    label, si01, si_raw0, (p1, q1), (p0, q0) = hierarchy(n_raw, 7 * n_raw + 1, sparse)
    want_v, want_r = materialised(label, si01, si_raw0)
    sub1, sub0 = cluster_of(p1, q1, dev), cluster_of(p0, q0, dev)
    rng = np.random.default_rng(n_raw)
    combos = {"ii": [si01.to(dev), si_raw0.to(dev)], "ic": [si01.to(dev), sub0],
              "ci": [sub1, si_raw0.to(dev)], "cc": [sub1, sub0]}
    for c in (1, 13, 32):
        y = torch.from_numpy(rng.integers(-1, c + 2, n_raw))              # void: -1, c, c + 1
        want_cm = ops.histogram_confusion_matrix(want_r, y, c)            # CPU tensors
        assert int(want_cm.sum()) == int(((y >= 0) & (y < c) & (want_r < c)).sum())
        for name, hops in combos.items():
            res = predict.labels_through(label.to(dev), hops, target=y.to(dev), num_classes=c)
            assert torch.equal(res["voxel"].cpu(), want_v), (name, c)
            assert torch.equal(res["raw"].cpu(), want_r), (name, c)
            assert torch.equal(res["confmat"].cpu(), want_cm), (name, c)
            # the evaluation case: nothing materialised, accumulated into what the matrix holds
            held = torch.full((c, c), 3, dtype=torch.int64, device=dev)
            only = predict.labels_through(label.to(dev), hops, target=y.to(dev), num_classes=c,
                                          confmat=held, want=())
            assert set(only) == {"confmat"} and only["confmat"] is held
            assert torch.equal(held.cpu(), want_cm + 3), (name, c)
    # one hop, both forms, with the matrix at the voxel level
    yv = torch.from_numpy(rng.integers(-1, 15, si01.numel()))
    want_cm = ops.histogram_confusion_matrix(want_v, yv, 13)
    for hop in (si01.to(dev), sub1):
        res = predict.labels_through(label.to(dev), [hop], target=yv.to(dev), num_classes=13)
        assert set(res) == {"voxel", "confmat"}
        assert torch.equal(res["voxel"].cpu(), want_v) and torch.equal(res["confmat"].cpu(), want_cm)


def test_labels_through_out_of_range_writes_minus_one_and_counts(dev):
    from superpoint_transformer_amd import ops, predict
    label, si01, si_raw0, (p1, q1), (p0, q0) = hierarchy(1025, 77)
    label = label % 13
    n_sp, n_vox = label.numel(), si01.numel()
    y = torch.from_numpy(np.random.default_rng(3).integers(0, 13, 1025))
    bad1 = si01.clone()
    bad1[[5, 100]] = torch.tensor([n_sp, -1])
    bad2 = si_raw0.clone()
    bad2[[0, 1024]] = torch.tensor([n_vox, -3])
    want_v = label[bad1.clamp(0, n_sp - 1)]
    want_v[[5, 100]] = -1
    want_r = want_v[bad2.clamp(0, n_vox - 1)]
    want_r[[0, 1024]] = -1
    want_cm = ops.histogram_confusion_matrix(want_r, y, 13)               # -1 stays out
    with pytest.raises(ValueError, match=rf"hop 1: 2 index entries outside \[0, {n_sp}\); "
                                         rf"hop 2: 2 index entries outside \[0, {n_vox}\)"):
        predict.labels_through(label.to(dev), [bad1.to(dev), bad2.to(dev)])
    res = predict.labels_through(label.to(dev), [bad1.to(dev), bad2.to(dev)], target=y.to(dev),
                                 num_classes=13, check=False)
    assert torch.equal(res["voxel"].cpu(), want_v) and torch.equal(res["raw"].cpu(), want_r)
    assert torch.equal(res["confmat"].cpu(), want_cm)
    # the same first hop in front of a Cluster
    sub0 = cluster_of(p0, q0, dev)
    with pytest.raises(ValueError, match=rf"hop 1: 2 index entries outside \[0, {n_sp}\)"):
        predict.labels_through(label.to(dev), [bad1.to(dev), sub0])
    res = predict.labels_through(label.to(dev), [bad1.to(dev), sub0], check=False)
    assert torch.equal(res["raw"].cpu(), want_v[si_raw0])
    # a Cluster whose points leave the range: counted, never written through
    pts = q0.clone()
    lost = [int(pts[10]), int(pts[900])]
    pts[10], pts[900] = 1025, -1
    with pytest.raises(ValueError, match=r"hop 2: 2 point\(s\) of the Cluster outside \[0, 1025\)"):
        predict.labels_through(label.to(dev), [si01.to(dev), cluster_of(p0, pts, dev)])
    # ... and pointers that are not monotone: counted, and every write stays inside the output
    ptr = p0.clone()
    assert int(ptr[n_vox // 2 - 1]) > 0
    ptr[n_vox // 2] = ptr[n_vox // 2 - 1] - 1
    with pytest.raises(ValueError, match="pointers are not a monotone"):
        predict.labels_through(label.to(dev), [si01.to(dev), cluster_of(ptr, q0, dev)])
    keep = torch.ones(1025, dtype=torch.bool)
    keep[lost] = False
    res = predict.labels_through(label.to(dev), [si01.to(dev), cluster_of(p0, pts, dev)], check=False)
    assert torch.equal(res["raw"].cpu()[keep], label[si01][si_raw0][keep])


# ---- capture ---------------------------------------------------------------------------------------
def test_check_false_pair_under_a_graph(dev):
    """labels_through(check=False) + row_argmax captured on one stream (a linear sequence) and
    replayed twice give the eager result."""
    from superpoint_transformer_amd import predict
    lab, si01, si_raw0, (p1, q1), (p0, q0) = hierarchy(4100, 11)
    n_sp = lab.numel()
    gen = torch.Generator().manual_seed(2)
    logits = torch.randn(n_sp, C, generator=gen).to(dev)
    y = torch.randint(0, 14, (4100,), generator=gen).to(dev)
    sub0 = cluster_of(p0, q0, dev)
    d_si01 = si01.to(dev)

    def pair(cm):
        pred = predict.row_argmax(logits)
        return predict.labels_through(pred, [d_si01, sub0], target=y, num_classes=C, confmat=cm,
                                      want=("raw",), check=False)

    eager = pair(torch.zeros(C, C, dtype=torch.int64, device=dev))           # (also the warm-up)
    torch.cuda.synchronize()
    cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = pair(cm)
    cm.zero_()
    for k in (1, 2):
        res["raw"].fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res["raw"], eager["raw"])
        assert torch.equal(cm, k * eager["confmat"])                      # accumulated per replay
    want = torch.argmax(logits.cpu(), dim=1)[si01][si_raw0]
    assert torch.equal(eager["raw"].cpu(), want)


# ---- the inference step --------------------------------------------------------------------------
def test_infer_step_output_full_resolution(dev):
    from superpoint_transformer_amd import hotpath
    from superpoint_transformer_amd.synthetic import make_nag
    nag = make_nag("R", seed=3, device=dev, sizes=(6000, 200, 80, 2500, 2000, 1))
    path = hotpath.SPTInferStep(nag, dev, seed=3)
    logits = path.step()
    out = path.output()
    assert out.num_nodes == 200 and not out.multi_stage and out.logits is logits[0]
    si01 = nag[0]["super_index"]
    gen = torch.Generator().manual_seed(4)
    si_raw0 = torch.randint(0, 6000, (15001,), generator=gen)
    si_raw0[-1] = 5999                                      # (the dense Cluster then has 6 000 rows)
    from superpoint_transformer_amd.data import Cluster
    sub0 = Cluster(si_raw0.to(dev), torch.arange(15001, device=dev), dense=True)
    assert sub0.num_clusters == 6000
    want = torch.argmax(logits[0].float().cpu(), dim=1)[si01.cpu()][si_raw0]
    for kw in (dict(super_index_raw_to_level0=si_raw0.to(dev)), dict(sub_level0_to_raw=sub0)):
        got = out.full_res_semantic_pred(super_index_level0_to_level1=si01, **kw)
        assert got.shape == (15001,) and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
