"""The entries of csrc/partition_loss.hip under tests/guarded.py, called through the C ABI: every
input flush against its guard (NaN behind floats, zero behind indices), every output cut to the
byte between guards and pre-filled with a sentinel, the workspace exactly what its query promises
and NaN-filled (0xFF: -1 as an index or a counter, NaN as a float).  Asked for: intact guards and
the bits of the plain run through the Python wrapper."""
import pytest
import torch

import panoptic_cases as pc
import partition_criterion_cases as cc
from test_panoptic_contract_gpu import arena_for, call, fresh, put, query

pytestmark = pytest.mark.gpu

PARAMS = (0.5, 2.0, 0.8, 1e-6)                     # temperature, gamma, weight, epsilon


def test_wrappers_on_exact_poisoned_memory(dev):
    """The Python surface once more with every ``_workspace`` request cut to the byte between
    guards and NaN-filled, and every fresh float tensor NaN-filled: the comparisons with the
    reference's fixture and the twin must hold unchanged."""
    from guarded import exact_workspaces, poisoned_fresh_tensors
    arena = arena_for(dev)
    with poisoned_fresh_tensors(dev), exact_workspaces(arena):
        cc.check_fixture(dev)
        cc.check_fake_losses(dev)
        cc.check_sampling(dev, 0.5)
        cc.check_criterion(dev)
    assert len(arena) > 0


@pytest.mark.parametrize("n,d,e", [(2, 32, 1), (90, 32, 255), (90, 7, 256), (90, 33, 257), (300, 128, 1030)])
@pytest.mark.parametrize("ratio", [None, 0.5])
def test_forward_and_backward_between_guards(n, d, e, ratio, dev):
    from superpoint_transformer_amd import csr, ops
    x, y, ei = cc.random_case(n, d, e, seed=n + d + e)
    if e == 1:
        ei[:] = [[0], [1]]
        y[:] = 0
        y[0, 1] = y[1, 2] = 3                       # one inter edge
    xt, yt, eit = (torch.from_numpy(a).to(dev) for a in (x, y, ei))
    xr = xt.clone().requires_grad_()
    want_counts = torch.zeros(3, dtype=torch.int64, device=dev)
    want_sel = torch.zeros(e, dtype=torch.uint8, device=dev)
    state = torch.tensor([9, 3], dtype=torch.int64, device=dev) if ratio else None
    want = ops.partition_edge_loss(xr, yt, eit, 5, *PARAMS, ratio=ratio, state=state,
                                   counts=want_counts, selected=want_sel)
    want_grad = torch.autograd.grad(want, xr, torch.tensor(0.75, device=dev))[0]
    by_src, by_tgt = csr.edge_end_views(eit, n)

    arena = arena_for(dev)
    dx, dy, dei = put(arena, xt, "x"), put(arena, yt, "y"), put(arena, eit, "edge_index")
    nbytes = query("spt_partition_loss_workspace_bytes", n, e)
    assert nbytes > 0
    ws = arena.take(nbytes, label="ws")
    loss = fresh(arena, 1, torch.float32, "loss")
    den = fresh(arena, 1, torch.float64, "den")
    code = fresh(arena, e, torch.uint8, "code", fill=7)
    counts = fresh(arena, 3, torch.int64, "counts")
    status = put(arena, torch.zeros(2, dtype=torch.int32, device=dev), "status")
    selected = fresh(arena, e, torch.uint8, "selected", fill=7)
    dstate = put(arena, torch.tensor([9, 3], dtype=torch.int64, device=dev), "state") if ratio else None
    call("spt_partition_loss_fwd_f32", dx, d, n, d, dy, 6, 5, dei, e, *PARAMS,
         -1.0 if ratio is None else ratio, dstate, loss, den, code, counts, status, selected, ws, nbytes)
    arena.check()
    assert pc.bits(loss) == pc.bits(want.detach().reshape(1))
    assert torch.equal(counts, want_counts) and torch.equal(selected, want_sel)
    assert torch.equal(code != 0, selected != 0) and int(code.max()) <= 2
    assert status.tolist()[0] == 0 and float(den) == (float(counts[2]) if counts[0] > 0 else 0.0)
    if ratio:
        assert dstate.tolist() == [9, 4]
    gout = put(arena, torch.tensor([0.75], device=dev), "gout")
    views = [put(arena, t, k) for t, k in ((by_src.rowptr, "src_rowptr"), (by_src.perm, "src_perm"),
                                           (by_tgt.rowptr, "tgt_rowptr"), (by_tgt.perm, "tgt_perm"))]
    gx = fresh(arena, n * d, torch.float32, "gx")
    call("spt_partition_loss_bwd_f32", dx, d, n, d, dei, e, code, *views, *PARAMS, gout, den, gx, d)
    arena.check()
    assert pc.bits(gx) == pc.bits(want_grad.reshape(-1)) and not bool(gx.isnan().any())
    # without the optional outputs: the same loss
    loss2 = fresh(arena, 1, torch.float32, "loss")
    if ratio:
        dstate.copy_(torch.tensor([9, 3], device=dev))
    call("spt_partition_loss_fwd_f32", dx, d, n, d, dy, 6, 5, dei, e, *PARAMS,
         -1.0 if ratio is None else ratio, dstate, loss2, den, code, None, None, None, ws, nbytes)
    arena.check()
    assert pc.bits(loss2) == pc.bits(loss)


def test_arguments_are_validated_before_any_launch(dev):
    from superpoint_transformer_amd import _lib
    L = _lib.lib
    assert L.spt_partition_loss_workspace_bytes(0, 5) == 0
    assert L.spt_partition_loss_workspace_bytes(5, 0) == 0
    assert L.spt_partition_loss_workspace_bytes(5, 1 << 31) == 0
    one = torch.zeros(64, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr(dev)
    p = one.data_ptr()
    big = 1 << 20
    fwd, bwd = L.spt_partition_loss_fwd_f32, L.spt_partition_loss_bwd_f32

    def refused(st, text):
        assert st != 0 and text in _lib.last_error(), _lib.last_error()

    ok = dict(T=1.0, g=0.0, w=0.5, eps=1e-6)
    refused(fwd(p, 129, 1, 129, p, 0, 5, p, 1, *ok.values(), -1.0, None, p, p, p, None, None, None,
                p, big, s), "wider than 128")
    refused(fwd(p, 32, 0, 32, p, 0, 5, p, 1, *ok.values(), -1.0, None, p, p, p, None, None, None,
                p, big, s), "1 <= N")
    refused(fwd(p, 16, 1, 32, p, 0, 5, p, 1, *ok.values(), -1.0, None, p, p, p, None, None, None,
                p, big, s), "stride")
    refused(fwd(p, 32, 1, 32, p, 3, 5, p, 1, *ok.values(), -1.0, None, p, p, p, None, None, None,
                p, big, s), "ycols")
    refused(fwd(p, 32, 1, 32, p, 0, 5, p, 1, 0.0, 0.0, 0.5, 1e-6, -1.0, None, p, p, p, None, None,
                None, p, big, s), "temperature")
    refused(fwd(p, 32, 1, 32, p, 0, 5, p, 1, *ok.values(), 0.0, p, p, p, p, None, None, None,
                p, big, s), "ratio")
    refused(fwd(p, 32, 1, 32, p, 0, 5, p, 1, *ok.values(), 0.5, None, p, p, p, None, None, None,
                p, big, s), "state")
    refused(fwd(p, 32, 1, 32, p, 0, 5, p, 1, *ok.values(), -1.0, None, p, p, None, None, None, None,
                p, big, s), "null pointer")
    refused(fwd(p, 32, 1, 32, p, 0, 5, p, 1, *ok.values(), -1.0, None, p, p, p, None, None, None,
                p, 64, s), "workspace too small")
    refused(bwd(p, 32, 1, 129, p, 1, p, p, p, p, p, *ok.values(), p, p, p, 129, s), "wider than 128")
    refused(bwd(p, 32, 1, 32, p, 1, p, p, p, p, None, *ok.values(), p, p, p, 32, s), "null pointer")
    refused(bwd(p, 32, 1, 32, p, 1, p, p, p, p, p, *ok.values(), p, p, p, 8, s), "stride")
    torch.cuda.synchronize(dev)
    assert not bool(one.any())
