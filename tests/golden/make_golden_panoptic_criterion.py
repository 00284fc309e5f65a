"""Golden fixture for the panoptic criterion, produced by the REFERENCE'S OWN code:

  * ``InstanceData.major`` (src/data/instance.py:162-225, the module imported verbatim as
    make_golden_instance.py does);
  * ``PanopticSegmentationOutput.void_mask`` / ``sanitized_edge_affinities``
    (src/utils/output_panoptic.py, imported verbatim);
  * ``BCEWithLogitsLoss`` / ``WeightedBCEWithLogitsLoss`` (src/loss/bce.py + weighted.py, loaded
    by file path);
  * ``PanopticSegmentationModule._edge_affinity_weights`` (src/models/panoptic.py:726-758), cut
    out of its class with ``ast`` - unmodified - and run on a stand-in holding ``hparams``;
  * the semantic part of the combined loss: ``loss_with_target_histogram`` and the multi-stage
    'ce_kl' branch, as make_golden_criterion.py runs them.

Stand-ins: torch_scatter / consecutive_cluster = the oracle's restatements.

Scene A (C = 13), planted clusters for ``major`` (asserted on what the reference returned):
  0 one pair; 1 a count tie between its first and its last pair (the first wins); 2 void-major
  at EXACTLY half (sets the reference's global branch); 3 void-major above half, label 13
  (reassigned only because of that branch); 4 all void, labels -1 / 13 / 14, its largest pair above half (takes its
  first pair with count 0); 5 void-major above half, label 14; 6 object ids >= 2^31; 7 a void pair of
  16 777 217 points out of 33 554 432: above half as integers, exactly 0.5 as the f32 quotient;
  8 a tie between a non-void first and a void last pair; then seeded clusters whose void pairs
  are never the largest, and seeded void-major clusters above half.
Scene B: scene A without clusters 2 and 7 - every void-major cluster is above half, the branch is
not taken and nothing is reassigned.
Scene C: 300 nodes, E = 3 * 256 + 17 edges, the loss in six settings (plain / weighted
[1, 1, 1, 1] / weighted [0.5, 4, 0, 2], each with pos_weight 1 and 2.5): losses and gradients in
f32 (``c__*``) and in f64 (``f64__c__*``, the yardstick), tp / fp / tn / fn in integers, and the
combined loss ``semantic + 10 * edge affinity``.  Case D: 5 edges, every one between void nodes
(plain settings: the reference's weighted loss asserts on an empty selection).

Usage (build container only): python tests/golden/make_golden_panoptic_criterion.py [--check]
(``--check``: regenerate and compare with the committed file array by array, bit for bit).
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_criterion as mgc  # noqa: E402
import make_golden_instance as mgi  # noqa: E402
import make_golden_select as mgs  # noqa: E402
import grid_sampling_reference as R  # noqa: E402

C = 13
NAME = "panoptic_criterion.npz"
BIG = 16_777_217
N_C, E_C, N2_C = 300, 3 * 256 + 17, 60
SETTINGS = {"plain": (False, None), "w1": (True, [1, 1, 1, 1]), "w2": (True, [0.5, 4, 0, 2])}
POS_WEIGHTS = {"pw1": 1.0, "pw25": 2.5}
LAMBDA = 10

# scene A's planted clusters: lists of (obj, count, y)
PLANTED = [
    [(1, 5, 0)],
    [(4, 7, 1), (7, 3, 3), (10, 7, 3)],
    [(19, 10, -1), (1, 4, 0), (13, 6, 4)],
    [(22, 11, 13), (1, 5, 0)],
    [(19, 3, -1), (22, 8, 13), (25, 2, 14)],
    [(25, 9, 14), (4, 2, 1)],
    [((1 << 31) + 5, 8, 5), ((1 << 33) + 1, 3, 6)],
    [(28, BIG, -1), (1, (1 << 25) - BIG, 0)],
    [(13, 6, 4), (19, 6, -1)],
]
AT_HALF = (2, 7)
VALID_OBJ = {1: 0, 4: 1, 7: 3, 10: 3, 13: 4, 16: 5, 31: 9, 34: 12}
VOID_OBJ = {19: -1, 22: 13, 25: 14}


def load_bce():
    """src/loss/weighted.py and bce.py by file path, under the names bce.py imports."""
    for name in ("weighted", "bce"):
        full = f"src.loss.{name}"
        spec = importlib.util.spec_from_file_location(full, os.path.join(mg.REF, "src", "loss", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        if "src.loss" not in sys.modules:
            pkg = types.ModuleType("src.loss")
            pkg.__path__ = []
            sys.modules["src.loss"] = pkg
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
    return sys.modules["src.loss.bce"]


def cut_weights():
    code = mgs.cut("src/models/panoptic.py", "PanopticSegmentationModule", "_edge_affinity_weights")
    ns = {"torch": torch}
    exec(compile(code, "panoptic.py", "exec"), ns)
    return ns["_edge_affinity_weights"]


def clusters_a(rng):
    cl = [list(c) for c in PLANTED]
    valid, void = sorted(VALID_OBJ), sorted(VOID_OBJ)
    for _ in range(24):                            # void pairs never the largest
        k = int(rng.integers(1, 5))
        objs = rng.permutation(valid)[:k]
        c = [(int(o), int(rng.integers(5, 50)), VALID_OBJ[int(o)]) for o in objs]
        if rng.random() < 0.4:
            o = int(rng.choice(void))
            c.insert(int(rng.integers(0, len(c) + 1)), (o, int(rng.integers(1, 5)), VOID_OBJ[o]))
        cl.append(c)
    for _ in range(6):                             # void-major, above half
        o, v = int(rng.choice(void)), int(rng.choice(valid))
        c = [(v, int(rng.integers(1, 20)), VALID_OBJ[v]), (o, int(rng.integers(60, 90)), VOID_OBJ[o])]
        cl.append(c if rng.random() < 0.5 else c[::-1])
    return cl


def to_csr(clusters):
    ptr = np.cumsum([0] + [len(c) for c in clusters]).astype(np.int64)
    flat = [p for c in clusters for p in c]
    obj, count, y = (np.array([p[k] for p in flat], dtype=np.int64) for k in range(3))
    return ptr, obj, count, y


def scene_major(ID, tag, clusters, out):
    T = torch.from_numpy
    ptr, obj, count, y = to_csr(clusters)
    d = ID(T(ptr), T(obj), T(count), T(y))
    o, c, yy = d.major(num_classes=C)
    out.update({f"{tag}_pointers": ptr, f"{tag}_obj": obj, f"{tag}_count": count, f"{tag}_y": y,
                f"{tag}_major_obj": o, f"{tag}_major_count": c, f"{tag}_major_y": yy})
    return o.tolist(), c.tolist(), yy.tolist()


def scene_c(rng):
    """Nodes (an InstanceData and its histograms), edges, affinities, logits."""
    n_obj = 40
    obj_y = rng.integers(0, C, n_obj)
    obj_y[rng.permutation(n_obj)[:10]] = rng.choice([-1, C, C + 1], 10)
    clusters = []
    for v in range(N_C):
        k = int(rng.integers(1, 4))
        objs = rng.permutation(n_obj)[:k]
        c = []
        for o in objs:
            yv = int(obj_y[o])
            if int(o) == 5:                        # one object under two labels
                yv = 2 if v % 2 else 3
            c.append((int(o) * 3 + 1, int(rng.integers(1, 60)), yv))
        clusters.append(c)
    for v in range(0, 40):                         # many nodes whose major object is object 5
        clusters[v] = [(5 * 3 + 1, 100, 2 if v % 2 else 3)] + [p for p in clusters[v] if p[0] != 16][:1]
    ei = np.stack([rng.integers(0, N_C, E_C), rng.integers(0, N_C, E_C)]).astype(np.int64)
    ei[:, :60] = rng.integers(0, 40, (2, 60))      # edges among the object-5 nodes
    loop = ei[0] == ei[1]
    ei[1, loop] = (ei[0, loop] + 1) % N_C
    ei = np.stack([ei.min(0), ei.max(0)])
    target = rng.random(E_C).astype(np.float32)
    pick = rng.permutation(E_C)
    target[pick[:150]] = 0.0
    target[pick[150:300]] = 1.0
    target[pick[300:340]] = 0.5
    logits = (rng.normal(size=E_C) * 3).astype(np.float32)
    for k, v in enumerate((0.0, 40.0, -40.0, 90.0, -90.0)):
        logits[pick[k::97][:6]] = v                # each special value under several targets
    # (semantic logits on a grid of 1 / 8: they compress, the fixture stays small)
    sem1 = (np.round(rng.normal(size=(N_C, C)) * 16) / 8).astype(np.float32)
    sem2 = (np.round(rng.normal(size=(N2_C, C)) * 16) / 8).astype(np.float32)
    super_index = rng.integers(0, N2_C, N_C).astype(np.int64)
    super_index[:N2_C] = np.arange(N2_C)
    return clusters, ei, target, logits, sem1, sem2, super_index


def edge_losses(bce, weights_fn, Output, d, y_hist, ei, target, logits, dtype, prefix, out,
                semantic=None, settings=SETTINGS):
    """Every setting on one precision: losses, gradients; returns the kept mask and the cases."""
    T = torch.from_numpy
    n = d.num_clusters
    keep = kinds = None
    for sname, (weighted, cw) in ((k, SETTINGS[k]) for k in settings):
        for pname, pw in POS_WEIGHTS.items():
            x = T(logits).to(dtype).requires_grad_()
            sem = [torch.zeros(h.shape[0], C) for h in y_hist] if isinstance(y_hist, list) \
                else torch.zeros(n, C)
            o = Output(sem, [], x, torch.ones(n, dtype=torch.long), y_hist=y_hist,
                       obj=d, obj_edge_index=T(ei), obj_edge_affinity=T(target).to(dtype),
                       pos=torch.zeros(n, 3), obj_pos=torch.zeros(n, 3))
            assert o.has_target
            pred, tgt, same_class, same_obj = o.sanitized_edge_affinities()
            holder = types.SimpleNamespace(hparams=types.SimpleNamespace(edge_affinity_loss_weights=cw))
            w = weights_fn(holder, same_class, same_obj)
            assert (w is None) == (cw is None)
            if w is not None:
                w = w.to(dtype)
            cls = bce.WeightedBCEWithLogitsLoss if weighted else bce.BCEWithLogitsLoss
            crit = cls(pos_weight=torch.tensor(pw, dtype=dtype))
            loss = crit(pred, tgt, w)
            grad = torch.autograd.grad(loss, x)[0] if pred.numel() else torch.zeros_like(x)
            out[f"{prefix}{sname}_{pname}_loss"] = loss.detach()
            out[f"{prefix}{sname}_{pname}_grad"] = grad
            if semantic is not None and sname == "plain" and pname == "pw1":
                out[f"{prefix}combined"] = (semantic + LAMBDA * loss).detach()
                out[f"{prefix}semantic"] = semantic.detach()
            if keep is None:
                keep = ~o.void_edge_mask
                kinds = 2 * (~same_class).long() + (~same_obj).long()
                void = o.void_mask
    return keep, kinds, void


def build():
    torch.set_num_threads(1)
    U, csr, inst = mgi.load_reference()
    ID = inst.InstanceData
    sys.modules["src.data"].InstanceData = ID
    Output = importlib.import_module("src.utils.output_panoptic").PanopticSegmentationOutput
    bce = load_bce()
    weights_fn = cut_weights()
    ref_loss = mgc.reference_loss_module()
    rng = np.random.default_rng(20261021)
    T = torch.from_numpy
    out = {"num_classes": np.int64(C)}

    # ---- scenes A and B: major ------------------------------------------------------------------
    cl_a = clusters_a(rng)
    cl_b = [c for k, c in enumerate(cl_a) if k not in AT_HALF]
    assert 38 <= len(cl_a) <= 42
    o, c, y = scene_major(ID, "a", cl_a, out)
    assert (o[0], c[0], y[0]) == (1, 5, 0)
    assert (o[1], c[1], y[1]) == (4, 7, 1)                           # the first of the tie
    assert (o[2], c[2], y[2]) == (13, 6, 4)                          # at half: second best
    assert (o[3], c[3], y[3]) == (1, 5, 0)                           # above half, reassigned all the same
    assert (o[4], c[4], y[4]) == (19, 0, -1)                         # all void: first pair, count 0
    assert (o[5], c[5], y[5]) == (4, 2, 1)
    assert (o[6], c[6], y[6]) == ((1 << 31) + 5, 8, 5)
    assert (o[7], c[7], y[7]) == (1, (1 << 25) - BIG, 0)             # 0.5 as f32, more as integers
    assert float(torch.tensor(BIG) / torch.tensor(1 << 25)) == 0.5 and 2 * BIG > (1 << 25)
    assert (o[8], c[8], y[8]) == (13, 6, 4)
    assert all(0 <= v < C for k, v in enumerate(y) if k != 4)        # every void-major one moved
    ob, cb, yb = scene_major(ID, "b", cl_b, out)
    assert (ob[2], cb[2], yb[2]) == (22, 11, 13)                     # cluster 3 of A keeps its void
    assert (ob[3], cb[3], yb[3]) == (22, 8, 13)                      # the all-void one its largest
    assert (ob[4], cb[4], yb[4]) == (25, 9, 14)
    assert sum(not 0 <= v < C for v in yb) == 3 + 6

    # ---- scene C: the loss ----------------------------------------------------------------------
    clusters, ei, target, logits, sem1, sem2, super_index = scene_c(rng)
    ptr, obj, count, y = to_csr(clusters)
    d = ID(T(ptr), T(obj), T(count), T(y))
    y1 = d.target_label_histogram(C)
    y2 = torch.zeros(N2_C, C + 1, dtype=torch.long).index_add_(0, T(super_index), y1)
    mo, mc, my = d.major(num_classes=C)
    out.update(c_pointers=ptr, c_obj=obj, c_count=count, c_y=y, c_y_hist1=y1.int(), c_y_hist2=y2.int(),
               c_edge_index=ei, c_target=target, c_logits=logits, c_sem1=sem1, c_sem2=sem2,
               c_major_obj=mo, c_major_y=my)
    semantic = {}
    for dtype, tag in ((torch.float32, "c__"), (torch.float64, "f64__c__")):
        criteria = [torch.nn.CrossEntropyLoss(ignore_index=C) for _ in mgc.LAMBDAS]
        semantic[tag] = mgc.multi_stage("ce_kl", ref_loss.loss_with_target_histogram, criteria,
                                        [T(sem1).to(dtype), T(sem2).to(dtype)], [y1, y2])
    keep, kinds, void = edge_losses(bce, weights_fn, Output, d, [y1, y2], ei, target, logits,
                                    torch.float32, "c__", out, semantic["c__"])
    edge_losses(bce, weights_fn, Output, d, [y1, y2], ei, target, logits, torch.float64,
                "f64__c__", out, semantic["f64__c__"])
    full_kinds = torch.full((E_C,), -1, dtype=torch.long)
    full_kinds[keep] = kinds
    out.update(c_void=void, c_keep=keep, c_kind=full_kinds)
    pred, tgt = T(logits)[keep] > 0, T(target)[keep] > 0.5
    stats = [int((pred & tgt).sum()), int((pred & ~tgt).sum()), int((~pred & ~tgt).sum()),
             int((~pred & tgt).sum())]
    out["c_stats"] = np.array(stats, dtype=np.int64)
    # what the scene was built to hold
    vi, vj = void[T(ei)[0]], void[T(ei)[1]]
    assert int((vi & vj).sum()) >= 5 and int((vi ^ vj).sum()) >= 50 and int((~vi & ~vj).sum()) >= 300
    assert sorted(set(kinds.tolist())) == [0, 1, 2, 3], sorted(set(kinds.tolist()))
    assert int((kinds == 2).sum()) >= 5                              # one object under two labels
    kt = T(target)[keep]
    assert all(int((kt == v).sum()) >= 10 for v in (0.0, 1.0, 0.5)) and int(((kt > 0) & (kt < 1)).sum()) > 100
    kl = T(logits)[keep]
    assert all(int((kl == v).sum()) >= 1 for v in (0.0, 40.0, -40.0, 90.0, -90.0))
    assert all(s > 0 for s in stats) and sum(stats) == int(keep.sum())
    for k, v in out.items():
        if k.endswith("_loss") or k.endswith("_grad"):
            assert bool(torch.isfinite(torch.as_tensor(v)).all()), k

    # ---- case D: every edge between two void nodes ----------------------------------------------
    cl_d = [[(19, 5, -1)], [(22, 7, 13), (1, 1, 0)], [(25, 3, 14)], [(1, 9, 0)]]
    ptr, obj, count, y = to_csr(cl_d)
    dd = ID(T(ptr), T(obj), T(count), T(y))
    yd = dd.target_label_histogram(C)
    ei_d = np.array([[0, 0, 1, 0, 1], [1, 2, 2, 1, 2]], dtype=np.int64)
    tg_d = np.array([0.0, 1.0, 0.5, 0.25, 1.0], dtype=np.float32)
    lg_d = np.array([0.5, -2.0, 90.0, 0.0, 3.0], dtype=np.float32)
    out.update(d_pointers=ptr, d_obj=obj, d_count=count, d_y=y, d_y_hist=yd.int(), d_edge_index=ei_d,
               d_target=tg_d, d_logits=lg_d)
    # (plain only: with a weight table the reference's WeightedLossMixIn asserts "At least one
    # weight must be non-zero" on the empty selection)
    keep_d, _, void_d = edge_losses(bce, weights_fn, Output, dd, yd, ei_d, tg_d, lg_d, torch.float32,
                                    "d__", out, settings=("plain",))
    assert not bool(keep_d.any()) and void_d.tolist() == [True, True, True, False]
    for pname in POS_WEIGHTS:
        assert bool(torch.isnan(out[f"d__plain_{pname}_loss"]))
        assert not bool(out[f"d__plain_{pname}_grad"].any())
    return out


def main():
    out = build()
    path = os.path.join(HERE, NAME)
    if "--check" in sys.argv:
        old = dict(np.load(path))
        assert set(old) == set(out), sorted(set(old) ^ set(out))
        for k, v in out.items():
            v = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
            assert R.bits_equal(old[k], v), f"{k} differs from the committed fixture"
        print(f"{NAME}: {len(out)} arrays bit-identical to the regenerated ones")
        return
    mg.save(NAME, **out)
    print(f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
