"""CPU suite: the torch composition of ``predict`` / ``output`` against every stored array of
tests/golden/semantic_output.npz, which the reference's own ``SemanticSegmentationOutput``,
``Cluster`` and multi-run helpers produced (tests/golden/make_golden_semantic_output.py).
Every comparison is exact: integers, booleans, and f32 sums formed by the same single adds."""
import logging
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN, load_golden
from superpoint_transformer_amd import output as out_mod
from superpoint_transformer_amd import predict
from superpoint_transformer_amd.data import NAG, Cluster, Data
from superpoint_transformer_amd.output import MultiRunInference, SemanticSegmentationOutput
from superpoint_transformer_amd.transforms import NAGSaveNodeIndex

C = 13
KEY = "tta_node_id"


@pytest.fixture(scope="module")
def g():
    return {k: torch.from_numpy(v) for k, v in load_golden("semantic_output.npz").items()}


def bits(a, b):
    """Same dtype, shape and bytes (NaN payloads and signed zeros included)."""
    return a.dtype == b.dtype and a.shape == b.shape and \
        a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes()


def outputs(g):
    return {"single": SemanticSegmentationOutput(g["in__logits_single"], g["in__y_hist"]),
            "multi": SemanticSegmentationOutput([g["in__logits_multi1"], g["in__logits_multi2"]],
                                                [g["in__y_hist"], g["in__y_hist"][:9]])}


def hops(g):
    return (g["in__si01"], g["in__si_raw0"],
            Cluster(g["in__sub1_pointers"], g["in__sub1_points"]),
            Cluster(g["in__sub0_pointers"], g["in__sub0_points"]))


def test_fixture_holds_what_it_claims(g):
    z = g["in__logits_single"]
    assert z[3].unique().numel() == 1 and bool(torch.isinf(z[4]).all())
    assert int(torch.isnan(z[5]).sum()) == 1 and int(torch.isnan(z[6]).sum()) == 2
    s1 = g["in__sub1_pointers"].diff()
    s0 = g["in__sub0_pointers"].diff()
    assert int(s1.max()) == 120 and (s1[[0, 18, 36]] == 0).all() and int((s1 == 1).sum()) >= 10
    assert int((s0 == 200).sum()) == 2 and (s0[[0, 128, 256]] == 0).all()
    assert g["in__si01"].numel() == 257 and g["in__si_raw0"].numel() == 1025
    for y in (g["in__y_voxel"], g["in__y_raw"]):
        assert int((y == 14).sum()) == 3 and int((y == -1).sum()) == 2 and int((y == 13).sum()) > 0
    for case in ("single", "multi"):
        assert int((~g[f"{case}__seen"]).sum()) == 5
        assert int((g[f"{case}__in__neighbors"] == -1).sum()) == 1
    assert "multi__in__batch" in g and "single__in__batch" not in g


def test_surface_and_predictions(g):
    for name, o in outputs(g).items():
        assert o.multi_stage == (name == "multi") and o.has_target
        assert o.num_classes == C and o.num_nodes == 37 and o.device == torch.device("cpu")
        level1 = o.logits[0] if o.multi_stage else o.logits
        pred = o.semantic_pred()
        assert torch.equal(pred, g[f"{name}__semantic_pred"])
        assert torch.equal(pred, torch.argmax(level1, dim=1))             # NaN rows included
        assert torch.equal(o.void_mask, g[f"{name}__void_mask"]) and o.void_mask.dtype == torch.bool
        assert torch.equal(o.semantic_target, g["in__y_hist"])
    assert SemanticSegmentationOutput(g["in__logits_single"]).void_mask is None
    pred, void = predict.row_argmax(g["in__logits_single"], g["in__y_hist"])
    assert torch.equal(pred, g["single__semantic_pred"]) and torch.equal(void, g["single__void_mask"])
    # the rows the histogram was planted for: exactly half, one over, empty, f32 rounding
    assert void[:4].tolist() == [False, True, False, False]


def test_both_forms_of_each_hop_agree(g):
    si01, si_raw0, sub1, sub0 = hops(g)
    for name, o in outputs(g).items():
        want_v, want_r = g[f"{name}__voxel_semantic_pred"], g[f"{name}__full_res_semantic_pred"]
        assert torch.equal(o.voxel_semantic_pred(super_index=si01), want_v)
        assert torch.equal(o.voxel_semantic_pred(sub=sub1), want_v)
        for kw in (dict(super_index_level0_to_level1=si01, super_index_raw_to_level0=si_raw0),
                   dict(sub_level1_to_level0=sub1, sub_level0_to_raw=sub0),
                   dict(super_index_level0_to_level1=si01, sub_level0_to_raw=sub0),
                   dict(sub_level1_to_level0=sub1, super_index_raw_to_level0=si_raw0)):
            assert torch.equal(o.full_res_semantic_pred(**kw), want_r), sorted(kw)
        # the Cluster walk equals the reference's route through to_super_index()
        assert torch.equal(sub1.to_super_index(), si01) and torch.equal(sub0.to_super_index(), si_raw0)
        both = predict.labels_through(o.semantic_pred(), [sub1, sub0])
        assert torch.equal(both["voxel"], want_v) and torch.equal(both["raw"], want_r)


def test_assertions_fire_without_a_hop(g):
    o = outputs(g)["single"]
    with pytest.raises(AssertionError, match="Must provide either `super_index` or `sub`"):
        o.voxel_semantic_pred()
    with pytest.raises(AssertionError, match="`super_index_level0_to_level1` or `sub_level1_to_level0`"):
        o.full_res_semantic_pred(super_index_raw_to_level0=g["in__si_raw0"])
    with pytest.raises(AssertionError, match="`super_index_raw_to_level0` or `sub_level0_to_raw`"):
        o.full_res_semantic_pred(super_index_level0_to_level1=g["in__si01"])
    with pytest.raises(AssertionError, match="Must provide either `super_index` or `sub`"):
        o.confusion_matrix(C, g["in__y_voxel"], resolution="voxel")


def test_confusion_matrices(g):
    from superpoint_transformer_amd import ops
    si01, si_raw0, sub1, sub0 = hops(g)
    for name, o in outputs(g).items():
        want_v, want_r = g[f"{name}__confmat_voxel"], g[f"{name}__confmat_raw"]
        for kw in (dict(super_index=si01), dict(sub=sub1)):
            assert torch.equal(o.confusion_matrix(C, g["in__y_voxel"], "voxel", **kw), want_v)
        for kw in (dict(super_index_level0_to_level1=si01, super_index_raw_to_level0=si_raw0),
                   dict(sub_level1_to_level0=sub1, sub_level0_to_raw=sub0),
                   dict(super_index_level0_to_level1=si01, sub_level0_to_raw=sub0),
                   dict(sub_level1_to_level0=sub1, super_index_raw_to_level0=si_raw0)):
            assert torch.equal(o.confusion_matrix(C, g["in__y_raw"], "raw", **kw), want_r)
        # conservation, and accumulation into a matrix that already holds counts
        y = g["in__y_raw"]
        assert int(want_r.sum()) == int(((y >= 0) & (y < C)).sum())
        acc = want_r.clone()
        res = o.confusion_matrix(C, y, "raw", out=acc, sub_level1_to_level0=sub1, sub_level0_to_raw=sub0)
        assert res is acc and torch.equal(acc, 2 * want_r)
        seg = o.confusion_matrix(C)
        assert torch.equal(seg, ops.histogram_confusion_matrix(o.semantic_pred(), g["in__y_hist"], C))


def test_out_of_range_is_reported_and_written_as_minus_one(g):
    si01, si_raw0, sub1, sub0 = hops(g)
    pred = g["single__semantic_pred"]
    bad1 = si01.clone()
    bad1[[3, 200]] = torch.tensor([37, -1])
    with pytest.raises(ValueError, match=r"hop 1: 2 index entries outside \[0, 37\)"):
        predict.labels_through(pred, [bad1, si_raw0])
    res = predict.labels_through(pred, [bad1, si_raw0], check=False)
    assert res["voxel"][[3, 200]].tolist() == [-1, -1]
    touched = (si_raw0 == 3) | (si_raw0 == 200)
    assert bool((res["raw"][touched] == -1).all())
    assert torch.equal(res["raw"][~touched], g["single__full_res_semantic_pred"][~touched])
    bad2 = si_raw0.clone()
    bad2[7] = 257
    with pytest.raises(ValueError, match=r"hop 2: 1 index entries outside \[0, 257\)"):
        predict.labels_through(pred, [si01, bad2])
    pts = g["in__sub0_points"].clone()
    pts[11] = 1025
    with pytest.raises(ValueError, match=r"hop 2: 1 point\(s\) of the Cluster outside \[0, 1025\)"):
        predict.labels_through(pred, [si01, Cluster(g["in__sub0_pointers"], pts)])
    ptr = g["in__sub0_pointers"].clone()
    ptr[40] = ptr[39] - 1
    with pytest.raises(ValueError, match="pointers are not a monotone"):
        predict.labels_through(pred, [si01, Cluster(ptr, g["in__sub0_points"])])


def test_accumulate_duplicate_and_out_of_range_raise():
    acc = torch.zeros(6, 3)
    stamp = torch.zeros(6, dtype=torch.int32)
    src = torch.arange(12.).view(4, 3)
    with pytest.raises(ValueError, match="1 node id.s. occur more than once in run 1"):
        predict.accumulate_rows_(acc, src, torch.tensor([2, 5, 2, 0]), stamp, 1)
    assert torch.equal(acc[2], src[0]) and torch.equal(acc[5], src[1]) and torch.equal(acc[0], src[3])
    with pytest.raises(ValueError, match=r"2 node id.s. lie outside \[0, 6\)"):
        predict.accumulate_rows_(acc, src, torch.tensor([6, 1, -1, 3]), stamp, 2)
    assert stamp.tolist() == [1, 2, 1, 2, 0, 1]
    assert torch.equal(acc[1], src[1]) and torch.equal(acc[4], torch.zeros(3))
    predict.accumulate_rows_(acc, src, torch.tensor([6, 1, 1, 3]), stamp, 3, check=False)   # silent
    with pytest.raises(ValueError, match="run >= 1"):
        predict.accumulate_rows_(acc, src, torch.tensor([0, 1, 2, 3]), stamp, 0)


def test_nag_save_node_index():
    nag = NAG([Data(pos=torch.zeros(n, 3)) for n in (7, 3, 2)])
    res = NAGSaveNodeIndex(key=KEY)(nag)
    assert res is nag
    for lv, n in zip(nag, (7, 3, 2)):
        assert torch.equal(lv[KEY], torch.arange(n)) and lv[KEY].dtype == torch.int64
    assert NAGSaveNodeIndex().key == "node_id"


def make_nag(g, case):
    lv1 = Data(pos=g[f"{case}__in__pos"].clone())
    if f"{case}__in__batch" in g:
        lv1.batch = g[f"{case}__in__batch"].clone()
    return NAG([Data(pos=torch.zeros(257, 3)), lv1, Data(pos=torch.zeros(9, 3))])


class DropNodes:
    """A stub transform: keeps the nodes of run ``r`` in the stored (shuffled) order, carrying
    every node attribute along - what a sampling augmentation does to a NAG."""

    def __init__(self, g, case, levels):
        self.g, self.case, self.levels, self.r = g, case, levels, 0
        self.transforms = [self._drop]

    def _drop(self, nag):
        for lv in range(1, self.levels + 1):
            keep = self.g[f"{self.case}__in__run{self.r}_node_id{lv}"]
            data = nag._list[lv]
            nag._list[lv] = Data(**{k: v[keep] for k, v in data})
        self.r += 1
        return nag

    def __call__(self, nag):
        for t in self.transforms:
            nag = t(nag)
        return nag


class StoredLogits:
    """A stub model: the stored logits of each run (one row per node the transform kept)."""

    def __init__(self, g, case, levels):
        self.g, self.case, self.levels, self.r, self.seen_ids = g, case, levels, 0, []

    def __call__(self, nag):
        z = [self.g[f"{self.case}__in__run{self.r}_logits{lv}"] for lv in range(1, self.levels + 1)]
        assert all(nag[lv][KEY].numel() == z[lv - 1].shape[0] for lv in range(1, self.levels + 1))
        self.seen_ids.append(nag[1][KEY].clone())
        self.r += 1
        return z if self.levels == 2 else z[0]


@pytest.mark.parametrize("case,levels", [("single", 1), ("multi", 2)])
def test_multi_run_steps_reproduce_the_stored_accumulation(g, case, levels):
    mri = MultiRunInference(C, multi_stage=levels == 2, key=KEY, r_max=2)
    nag = make_nag(g, case)
    om = mri.empty_output(nag)
    assert om.multi_stage == (levels == 2)
    for r in range(3):
        z = [g[f"{case}__in__run{r}_logits{lv}"] for lv in range(1, levels + 1)]
        ids = [None] + [{KEY: g[f"{case}__in__run{r}_node_id{lv}"]} for lv in range(1, levels + 1)]
        mri.update(om, SemanticSegmentationOutput(z if levels == 2 else z[0]), ids)
        acc = om.logits if levels == 2 else [om.logits]
        for lv in range(levels):
            assert bits(acc[lv], g[f"{case}__acc_run{r}_level{lv + 1}"]), (r, lv)
        # the stamp holds the last run that wrote each row
        last = torch.zeros(37, dtype=torch.int32)
        for q in range(r + 1):
            last[g[f"{case}__in__run{q}_node_id1"]] = q + 1
        assert torch.equal(om._tta_stamps[0], last)
    assert torch.equal(mri.seen(om), g[f"{case}__seen"])
    before2 = om.logits[1].clone() if levels == 2 else None
    # with the stored search result, and with the search of the CPU composition
    for neighbors in (g[f"{case}__in__neighbors"], None):
        om_k = SemanticSegmentationOutput([l.clone() for l in om.logits] if levels == 2 else om.logits.clone())
        om_k._tta_stamps, om_k._tta_run = om._tta_stamps, om._tta_run
        mri.finalize(om_k, nag, neighbors=neighbors)
        fin = om_k.logits if levels == 2 else [om_k.logits]
        for lv in range(levels):
            assert bits(fin[lv], g[f"{case}__final_level{lv + 1}"]), lv
        if levels == 2:
            assert bits(fin[1], before2)                    # level 1 only, like the reference


@pytest.mark.parametrize("case,levels", [("single", 1), ("multi", 2)])
def test_multi_run_loop_with_stub_model_and_transform(g, case, levels, caplog):
    mri = MultiRunInference(C, multi_stage=levels == 2, key=KEY, r_max=2)
    nag = make_nag(g, case)
    transform, model = DropNodes(g, case, levels), StoredLogits(g, case, levels)
    with caplog.at_level(logging.WARNING, logger=out_mod.__name__):
        om = mri.run(model, nag, transform, 3)
    fin = om.logits if levels == 2 else [om.logits]
    for lv in range(levels):
        assert bits(fin[lv], g[f"{case}__final_level{lv + 1}"]), lv
    # the transform list is as it was, the input NAG untouched, the ids went through the transform
    assert len(transform.transforms) == 1 and KEY not in nag[1]
    for r in range(3):
        assert torch.equal(model.seen_ids[r], g[f"{case}__in__run{r}_node_id1"])
    # the left-out node took the LAST seen row, and the warning states the counts
    far = int(torch.where(~g[f"{case}__seen"])[0][g[f"{case}__in__neighbors"] == -1])
    last_seen = int(torch.where(g[f"{case}__seen"])[0][-1])
    assert bits(fin[0][far], fin[0][last_seen])
    text = " ".join(r.getMessage() for r in caplog.records)
    assert "num_seen=32" in text and "num_unseen=5" in text and "num_left_out=1" in text
    assert "LAST seen" in text


def test_entries_validate_arguments_before_any_device_access():
    """Host only: every call below fails its argument checks, so the made-up pointers (8) are never
    dereferenced and no kernel is launched."""
    from superpoint_transformer_amd import _lib
    L = _lib.lib
    assert L.spt_row_argmax_f32(None, 5, 13, None, 0, None, None, None) != 0
    assert "nothing to compute" in _lib.last_error()
    assert L.spt_row_argmax_f32(None, -1, 13, None, 0, 8, None, None) != 0
    assert L.spt_rows_accumulate_f32(8, 4, 8, 8, 4, 3, 8, 0, 8, None) != 0 and "run >= 1" in _lib.last_error()
    assert L.spt_rows_accumulate_f32(None, 4, 8, 8, 4, 3, 8, 1, 8, None) != 0 and "null" in _lib.last_error()
    assert L.spt_labels_by_index_i64(8, 4, 8, 4, None, 0, 8, None, 8, 33, 8, 8, None) != 0
    assert "C <= 32" in _lib.last_error()
    assert L.spt_labels_by_index_i64(8, 4, 8, 4, None, 0, 8, None, 8, 13, None, 8, None) != 0
    assert "come together" in _lib.last_error()
    assert L.spt_labels_by_cluster_i64(8, 4, None, 8, 8, -1, 4, 8, None, 0, None, 8, None) != 0
    assert L.spt_labels_by_cluster_i64(8, 4, None, None, 8, 4, 4, 8, None, 0, None, 8, None) != 0
    assert "null" in _lib.last_error()


def test_generator_check_reproduces_the_committed_fixture():
    import re
    ref = re.search(r'^REF = "(.*)"$', open(os.path.join(GOLDEN, "make_golden.py")).read(), re.M).group(1)
    if not os.path.isdir(os.path.join(ref, "src")):
        pytest.skip("the reference tree the generator reads is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_semantic_output.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit-identical" in r.stdout
