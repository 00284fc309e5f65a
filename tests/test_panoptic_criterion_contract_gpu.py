"""The entries of the panoptic criterion (``spt_instance_major_i64`` of csrc/panoptic.hip,
``spt_edge_affinity_loss_{fwd,bwd}_f32`` of csrc/loss.hip) under tests/guarded.py, called through
the C ABI: every input flush against its guard (NaN behind floats, zero behind indices), every
output cut to the byte between guards and pre-filled with a sentinel, the workspace exactly what
its query promises and NaN-filled (0xFF: -1 as an index or a flag, NaN as a float).  Asked for:
intact guards and the bits of the plain run through the Python wrappers."""
import pytest
import torch

import panoptic_cases as pc
import panoptic_criterion_cases as cc
from test_panoptic_contract_gpu import arena_for, call, fresh, placed, put, query

pytestmark = pytest.mark.gpu


def test_wrappers_on_exact_poisoned_memory(dev):
    """The Python surface once more with every ``_workspace`` request cut to the byte between
    guards and NaN-filled, and every fresh float tensor NaN-filled: the comparisons with the
    reference's fixture must hold unchanged."""
    from guarded import exact_workspaces, poisoned_fresh_tensors
    arena = arena_for(dev)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        cc.check_major(dev)
        cc.check_masks_and_cases(dev)
        cc.check_losses(dev)
        cc.check_combined(dev)
        cc.check_all_void(dev)
        cc.check_metric(dev)
    assert len(arena) > 0


# one cluster with one pair; 65 pairs: one past a wave (the wave search), next to 64 (the lane
# search); more than one workgroup of clusters
MAJOR_CASES = [(1, 1), (3, 65), (5, 64), (17, 70), (700, 3)]


@pytest.mark.parametrize("g,per_cluster", MAJOR_CASES)
def test_major_objects_between_guards(g, per_cluster, dev):
    from superpoint_transformer_amd import panoptic
    d = pc.random_instance(g, per_cluster, cc.C, seed=3 * g + per_cluster).to(dev)
    want = panoptic.major_objects(d, cc.C, check=False)
    arena = arena_for(dev)
    ptr, obj, count, y = placed(arena, d)
    nbytes = query("spt_instance_major_workspace_bytes", g)
    assert nbytes > 0
    ws = arena.take(nbytes, label="ws")
    out = [fresh(arena, g, torch.int64, n) for n in ("out_obj", "out_count", "out_y")]
    status = put(arena, torch.zeros(2, dtype=torch.int32, device=dev), "status")
    call("spt_instance_major_i64", ptr, obj, count, y, g, d.num_items, cc.C, *out, status, ws,
         nbytes)
    arena.check()
    for got, exp in zip(out, want):
        assert torch.equal(got, exp)
    assert status.tolist() == [0, 0]
    for a, b in zip(want, d.major(cc.C)):                    # and the yardstick
        assert torch.equal(a, b)


@pytest.mark.parametrize("e", [1, 255, 256, 257])
@pytest.mark.parametrize("weighted", [False, True])
def test_edge_affinity_loss_between_guards(e, weighted, dev):
    from superpoint_transformer_amd import ops, panoptic, predict
    g = 1 if e == 1 else 40
    d, hist, ei, target, logits = cc.random_case(g, 1 if e == 1 else 3, e, seed=e, dev=dev)
    if e == 1:
        hist[:, cc.C] = 0                                    # the one edge is kept
    obj, _, y = panoptic.major_objects(d, cc.C, check=False)
    void = predict.void_mask(hist)
    cw = torch.tensor([0.5, 4.0, 0.25, 2.0], device=dev) if weighted else None
    pw = torch.tensor([2.5], device=dev) if weighted else None
    x = logits.clone().requires_grad_()
    want_stats = torch.zeros(4, dtype=torch.int64, device=dev)
    want = ops.edge_affinity_loss(x, target, ei, void, obj, y, case_weights=cw, pos_weight=pw,
                                  stats=want_stats)
    want_grad = torch.autograd.grad(want, x, torch.tensor(0.75, device=dev))[0]

    arena = arena_for(dev)
    dl, dt = put(arena, logits, "logits"), put(arena, target, "target")
    dei = put(arena, ei.contiguous(), "edge_index")
    dvoid = put(arena, void.to(torch.uint8), "node_void")
    dobj, dy = put(arena, obj, "node_obj"), put(arena, y, "node_y")
    dcw = put(arena, cw, "case_weight") if weighted else None
    dpw = put(arena, pw, "pos_weight") if weighted else None
    nbytes = query("spt_edge_affinity_loss_workspace_bytes", e)
    assert nbytes == 16 * ((e + 255) // 256)
    ws = arena.take(nbytes, label="ws")
    loss = fresh(arena, 1, torch.float32, "loss")
    den = fresh(arena, 1, torch.float64, "den")
    stats = put(arena, torch.zeros(4, dtype=torch.int64, device=dev), "stats")
    status = put(arena, torch.zeros(1, dtype=torch.int32, device=dev), "status")
    call("spt_edge_affinity_loss_fwd_f32", dl, dt, dei, e, dvoid, dobj, dy, g, dcw, dpw, loss, den,
         stats, status, ws, nbytes)
    arena.check()
    assert pc.bits(loss) == pc.bits(want.detach().reshape(1))
    assert torch.equal(stats, want_stats) and status.tolist() == [0]
    gout = put(arena, torch.tensor([0.75], device=dev), "gout")
    glog = fresh(arena, e, torch.float32, "glogits")
    call("spt_edge_affinity_loss_bwd_f32", dl, dt, dei, e, dvoid, dobj, dy, g, dcw, dpw, gout, den,
         glog)
    arena.check()
    assert pc.bits(glog) == pc.bits(want_grad) and not bool(glog.isnan().any())
    # without the optional outputs: the same loss
    loss2 = fresh(arena, 1, torch.float32, "loss")
    call("spt_edge_affinity_loss_fwd_f32", dl, dt, dei, e, dvoid, dobj, dy, g, dcw, dpw, loss2, den,
         None, None, ws, nbytes)
    arena.check()
    assert pc.bits(loss2) == pc.bits(loss)


def test_arguments_are_validated_before_any_launch(dev):
    from superpoint_transformer_amd import _lib
    L = _lib.lib
    assert L.spt_instance_major_workspace_bytes(0) == 0
    assert L.spt_edge_affinity_loss_workspace_bytes(0) == 0
    one = torch.zeros(8, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr(dev)
    p = one.data_ptr()
    assert L.spt_instance_major_i64(p, p, p, p, 1, 1, 13, p, p, p, p, p, 8, s) != 0      # small ws
    assert L.spt_instance_major_i64(p, p, p, p, 1, 1, 13, p, p, p, None, p, 1 << 20, s) != 0
    assert L.spt_edge_affinity_loss_fwd_f32(p, p, p, 1, p, p, p, 0, None, None, p, p, None, None,
                                            p, 64, s) != 0                               # N = 0
    assert L.spt_edge_affinity_loss_fwd_f32(p, p, p, 1, p, p, p, 1, None, None, p, p, None, None,
                                            p, 8, s) != 0                                # small ws
    assert L.spt_edge_affinity_loss_bwd_f32(p, p, p, 1, p, p, p, 1, None, None, p, None, p, s) != 0
    torch.cuda.synchronize(dev)
    assert not bool(one.any())
