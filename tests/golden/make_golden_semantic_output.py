"""Golden fixture for the way back from logits to the cloud, produced by the REFERENCE'S OWN
``SemanticSegmentationOutput`` (src/utils/output_semantic.py, imported verbatim), the three
helpers of its multi-run inference ``_create_empty_output``, ``_update_output_multi`` and
``_propagate_output_to_unseen_neighbors`` (src/models/semantic.py:563-616, cut out of the file
with ``ast`` - unmodified - because the module pulls Lightning at import) and its ``Cluster``
(src/data/cluster.py, loaded as make_golden_instance.py does).

Stand-ins: the ``knn_2(k=1, r_max=2)`` result is the exhaustive search of oracle/spt_oracle.py
on positions shifted per batch item as the reference's ``knn_2`` shifts them ("[third-party
restated]": FRNN runs on CUDA only); it is stored as an INPUT.  The NAG is a duck-typed list.
The confusion matrices are counted in numpy from the reference's predictions.

Contents (every array an input ``in__*`` or a result of the reference's code):
  * logits: single-stage [37, 13], multi-stage [[37, 13], [9, 13]], with planted ties (the first,
    a middle and the last column taking part), an all-equal row, a -inf row, a row with one NaN
    and a row with two;
  * y_hist [37, 14]: a row at exactly half void, one a count over half, one empty (0 / 0) and
    one whose counts exceed 2^24, where the f32 conversion rounds;
  * hierarchy 37 superpoints -> 257 voxels -> 1 025 raw points as ``super_index`` tensors and as
    Clusters with shuffled ``points``: one superpoint of 120 voxels among singletons, two voxels
    of 200 raw points, an empty cluster at the front, in the middle and at the end of both;
  * voxel and raw labels in [0, 13] (13 = void) with a few at 14 and -1;
  * multi-run cases ``single`` (single-stage, no batch) and ``multi`` (multi-stage, with batch):
    three runs over shuffled subsets of the nodes, five level-1 nodes never seen, one of them
    without a seen neighbour within r_max (``neighbors == -1``); the accumulated logits after
    each run, ``seen`` and the logits after propagation.

Usage (build container only): python tests/golden/make_golden_semantic_output.py [--check]
(``--check``: regenerate and compare with the committed file array by array, bit for bit).
"""
import ast
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_instance as mgi  # noqa: E402
import grid_sampling_reference as R  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

REF = mg.REF
C = 13
N1, N2, NV, NR = 37, 9, 257, 1025
KEY = "tta_node_id"
R_MAX = 2
UNSEEN = (4, 11, 20, 29, 33)       # level-1 nodes that no run samples; 33 sits far from all
FAR = 33


def load_reference():
    mgi.load_reference()
    cluster = sys.modules["src.data.cluster"]
    out = importlib.import_module("src.utils.output_semantic")
    tree = ast.parse(open(os.path.join(REF, "src/models/semantic.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SemanticSegmentationModule")
    names = ("_create_empty_output", "_update_output_multi", "_propagate_output_to_unseen_neighbors")
    body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == 3
    for n in body:
        n.decorator_list = []                      # (staticmethod: called as plain functions)
    ns = {"torch": torch, "NAG": object,
          "SemanticSegmentationOutput": out.SemanticSegmentationOutput}
    exec(compile(ast.Module(body=body, type_ignores=[]), "semantic.py", "exec"), ns)
    return out.SemanticSegmentationOutput, cluster.Cluster, [ns[n] for n in names]


class DuckNAG(list):
    """``nag[i]`` -> a namespace / dict of the level; ``num_points``; ``device``."""
    device = torch.device("cpu")

    @property
    def num_points(self):
        return [lv["n"] for lv in self]


def plant(logits):
    z = logits
    z[0, 0] = z[0, 5] = z[0].max() + 1            # tie, the first column wins
    z[1, 6] = z[1, 9] = z[1].max() + 1            # tie in the middle
    z[2, 7] = z[2, 12] = z[2].max() + 1           # tie with the last column
    z[7, 12] = z[7].max() + 1                     # the last column alone
    z[3] = 0.25                                   # all equal
    z[4] = -np.inf                                # all -inf
    z[5, 1] = 100.0
    z[5, 4] = np.nan                              # a NaN after a large number
    z[6, 2] = z[6, 9] = np.nan                    # two NaNs: the first wins
    return z


def split_sizes(rng, total, n, big, empty):
    """n sizes summing to total: ``big`` {index: size}, ``empty`` indices at 0, the rest >= 1
    with a good share of singletons."""
    sizes = np.ones(n, dtype=np.int64)
    for i in empty:
        sizes[i] = 0
    for i, s in big.items():
        sizes[i] = s
    free = [i for i in range(n) if i not in empty and i not in big]
    growers = free[::2]                           # every other one stays a singleton
    left = total - int(sizes.sum())
    assert left >= 0
    for i in rng.choice(growers, left):
        sizes[i] += 1
    assert int(sizes.sum()) == total
    return sizes


def make_hop(rng, sizes):
    """(super_index [sum], pointers, shuffled points) of clusters with these sizes."""
    total = int(sizes.sum())
    si = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(total)]
    pointers = np.concatenate(([0], np.cumsum(sizes)))
    points = np.argsort(si, kind="stable")
    for a, b in zip(pointers[:-1], pointers[1:]):
        points[a:b] = points[a:b][rng.permutation(b - a)]
    return si.astype(np.int64), pointers.astype(np.int64), points.astype(np.int64)


def labels(rng, n):
    y = rng.integers(0, C + 1, n).astype(np.int64)
    y[rng.choice(n, 5, replace=False)] = np.array([14, 14, -1, -1, 14])
    return y


def confusion(pred, y):
    cm = np.zeros((C, C), dtype=np.int64)
    ok = (y >= 0) & (y < C)
    np.add.at(cm, (y[ok], pred[ok]), 1)
    return cm


def nearest_seen(pos, batch, seen):
    """The stand-in for knn_2(x_search, x_query, 1, r_max=2, batch_search, batch_query)[0]."""
    seen_idx, unseen_idx = torch.where(seen)[0], torch.where(~seen)[0]
    x_search, x_query = pos[seen_idx].clone(), pos[unseen_idx].clone()
    if batch is not None:
        hi = max(x_search[:, 2].max(), x_query[:, 2].max())
        lo = min(x_search[:, 2].min(), x_query[:, 2].min())
        z_offset = hi - lo + R_MAX + 1
        x_search[:, 2] += batch[seen_idx] * z_offset
        x_query[:, 2] += batch[unseen_idx] * z_offset
    nb, _ = O.knn_brute_force(x_search, x_query, 1, r_max=R_MAX)
    return nb[:, 0]


def multi_run(rng, Output, helpers, case, multi_stage, with_batch):
    create, update, propagate = helpers
    out = {}
    pos = rng.uniform([0, 0, 0], [6, 6, 1], (N1, 3)).astype(np.float32)
    pos[FAR] = (100.0, 100.0, 0.0)
    batch = None
    if with_batch:
        batch = (np.arange(N1) % 2).astype(np.int64)
        # an unseen node whose nearest node in space belongs to the other batch item
        pos[UNSEEN[0]] = pos[UNSEEN[0] + 1] + np.float32(0.01)
        assert batch[UNSEEN[0]] != batch[UNSEEN[0] + 1]
        out[f"{case}__in__batch"] = batch
    out[f"{case}__in__pos"] = pos
    nag = DuckNAG([{"n": NV}, {"n": N1}, {"n": N2}])
    module = types.SimpleNamespace(num_classes=C, multi_stage_loss=multi_stage)
    output_multi = create(module, nag)
    seen = torch.zeros(N1, dtype=torch.bool)
    allowed = [np.array([i for i in range(N1) if i not in UNSEEN]), np.arange(N2)]
    levels = 2 if multi_stage else 1
    for r in range(3):
        ids, run_logits = [], []
        for lv in range(levels):
            pool = allowed[lv]
            k = int(rng.integers(len(pool) // 2, len(pool) + 1))
            pick = rng.permutation(pool)[:k]
            if lv == 0 and r == 2:                 # the last run sees what the others missed
                missed = np.array([i for i in pool if not bool(seen[i]) and i not in pick],
                                  dtype=pick.dtype)
                pick = rng.permutation(np.concatenate((pick, missed)))
            ids.append(pick.astype(np.int64))
            run_logits.append(rng.normal(size=(k, C)).astype(np.float32))
            out[f"{case}__in__run{r}_node_id{lv + 1}"] = ids[-1]
            out[f"{case}__in__run{r}_logits{lv + 1}"] = run_logits[-1]
        nag_t = [None] + [{KEY: torch.from_numpy(i)} for i in ids]
        t = [torch.from_numpy(z) for z in run_logits]
        output = Output(t if multi_stage else t[0])
        output_multi = update(output_multi, nag, output, nag_t, KEY)
        seen[nag_t[1][KEY]] = True
        acc = output_multi.logits if multi_stage else [output_multi.logits]
        for lv in range(levels):
            out[f"{case}__acc_run{r}_level{lv + 1}"] = acc[lv].clone().numpy()
    assert sorted(torch.where(~seen)[0].tolist()) == sorted(UNSEEN)
    tpos = torch.from_numpy(pos)
    neighbors = nearest_seen(tpos, None if batch is None else torch.from_numpy(batch), seen)
    assert int((neighbors == -1).sum()) == 1
    if with_batch:                                 # the batch vector changes the first answer
        assert not torch.equal(neighbors, nearest_seen(tpos, None, seen))
    out[f"{case}__seen"] = seen.numpy()
    out[f"{case}__in__neighbors"] = neighbors.numpy()
    output_multi = propagate(output_multi, nag, seen, neighbors)
    fin = output_multi.logits if multi_stage else [output_multi.logits]
    for lv in range(levels):
        out[f"{case}__final_level{lv + 1}"] = fin[lv].numpy()
    # what the reference does for neighbors == -1: the LAST seen row
    last_seen = int(torch.where(seen)[0][-1])
    assert np.array_equal(fin[0][FAR].numpy(), fin[0][last_seen].numpy())
    return out


def build():
    torch.set_num_threads(1)
    Output, Cluster, helpers = load_reference()
    rng = np.random.default_rng(20251019)
    out = {}

    single = plant(rng.normal(size=(N1, C)).astype(np.float32))
    multi1 = plant(rng.normal(size=(N1, C)).astype(np.float32))
    multi2 = rng.normal(size=(N2, C)).astype(np.float32)
    multi2[2, 3] = multi2[2, 8] = 9.0
    out.update(in__logits_single=single, in__logits_multi1=multi1, in__logits_multi2=multi2)

    y_hist = rng.integers(0, 20, (N1, C + 1)).astype(np.int64)
    y_hist[0] = 0
    y_hist[0, 2], y_hist[0, -1] = 10, 10                     # exactly half: not void
    y_hist[1] = 0
    y_hist[1, 5], y_hist[1, -1] = 10, 11                     # one count over half: void
    y_hist[2] = 0                                            # 0 / 0 = NaN: not void
    y_hist[3] = 0
    y_hist[3, 0], y_hist[3, -1] = (1 << 24), (1 << 24) + 1   # over half, f32 says exactly half
    out["in__y_hist"] = y_hist
    y_hist2 = rng.integers(0, 50, (N2, C + 1)).astype(np.int64)

    s1 = split_sizes(rng, NV, N1, {5: 120}, (0, 18, 36))
    s0 = split_sizes(rng, NR, NV, {7: 200, 130: 200}, (0, 128, 256))
    si01, ptr1, pts1 = make_hop(rng, s1)
    si_raw0, ptr0, pts0 = make_hop(rng, s0)
    out.update(in__si01=si01, in__sub1_pointers=ptr1, in__sub1_points=pts1,
               in__si_raw0=si_raw0, in__sub0_pointers=ptr0, in__sub0_points=pts0)
    sub1 = Cluster(torch.from_numpy(ptr1), torch.from_numpy(pts1))
    sub0 = Cluster(torch.from_numpy(ptr0), torch.from_numpy(pts0))
    assert torch.equal(sub1.to_super_index(), torch.from_numpy(si01))
    assert torch.equal(sub0.to_super_index(), torch.from_numpy(si_raw0))
    y_voxel, y_raw = labels(rng, NV), labels(rng, NR)
    out.update(in__y_voxel=y_voxel, in__y_raw=y_raw)

    t_si01, t_si_raw0 = torch.from_numpy(si01), torch.from_numpy(si_raw0)
    cases = {"single": Output(torch.from_numpy(single), torch.from_numpy(y_hist)),
             "multi": Output([torch.from_numpy(multi1), torch.from_numpy(multi2)],
                             [torch.from_numpy(y_hist), torch.from_numpy(y_hist2)])}
    for name, o in cases.items():
        pred = o.semantic_pred()
        voxel = o.voxel_semantic_pred(super_index=t_si01)
        assert torch.equal(voxel, o.voxel_semantic_pred(sub=sub1))
        raw = o.full_res_semantic_pred(super_index_level0_to_level1=t_si01,
                                       super_index_raw_to_level0=t_si_raw0)
        for kw in (dict(sub_level1_to_level0=sub1, sub_level0_to_raw=sub0),
                   dict(super_index_level0_to_level1=t_si01, sub_level0_to_raw=sub0),
                   dict(sub_level1_to_level0=sub1, super_index_raw_to_level0=t_si_raw0)):
            assert torch.equal(raw, o.full_res_semantic_pred(**kw))
        out[f"{name}__semantic_pred"] = pred.numpy()
        out[f"{name}__void_mask"] = o.void_mask.numpy()
        out[f"{name}__voxel_semantic_pred"] = voxel.numpy()
        out[f"{name}__full_res_semantic_pred"] = raw.numpy()
        out[f"{name}__confmat_voxel"] = confusion(voxel.numpy(), y_voxel)
        out[f"{name}__confmat_raw"] = confusion(raw.numpy(), y_raw)
    p = out["single__semantic_pred"]
    assert list(p[:8]) == [0, 6, 7, 0, 0, 4, 2, 12], p[:8]
    assert list(out["single__void_mask"][:4]) == [False, True, False, False]

    out.update(multi_run(rng, Output, helpers, "single", False, False))
    out.update(multi_run(rng, Output, helpers, "multi", True, True))
    return out


def main():
    out = build()
    path = os.path.join(HERE, "semantic_output.npz")
    if "--check" in sys.argv:
        old = dict(np.load(path))
        assert set(old) == set(out), sorted(set(old) ^ set(out))
        for k, v in out.items():
            v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
            assert R.bits_equal(old[k], v), f"{k} differs from the committed fixture"
        print(f"semantic_output.npz: {len(out)} arrays bit-identical to the regenerated ones")
        return
    mg.save("semantic_output.npz", **out)
    print(f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
