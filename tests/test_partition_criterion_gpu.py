"""The partition criterion on the device - csrc/partition_loss.hip through
``ops.partition_edge_loss`` and ``criterion.PartitionCriterion`` - against the reference's own
output (tests/golden/partition_criterion.npz) and the float64 host twin
(tests/partition_criterion_reference.py).  tests/partition_criterion_cases.py holds the
comparisons the CPU route shares."""
import numpy as np
import pytest
import torch

import panoptic_cases as pc
import partition_criterion_cases as cc

pytestmark = pytest.mark.gpu


def test_losses_gradients_and_counters_in_every_setting(dev):
    cc.check_fixture(dev)


def test_all_void_and_single_label_give_exactly_zero(dev):
    cc.check_fake_losses(dev)


def test_label_vector_decides_like_the_histograms(dev):
    cc.check_label_vector(dev)


@pytest.mark.parametrize("ratio", cc.RATIOS)
def test_sample_equals_the_twins(ratio, dev):
    cc.check_sampling(dev, ratio)


def test_criterion_on_a_partition_output(dev):
    cc.check_criterion(dev)


def test_arguments_are_refused(dev):
    cc.check_arguments(dev)


# 1, 7: scalar loads; 32: one 8-lane pass of float4; 33: a second pass with one column, scalar;
# 64, 128: two and four passes
@pytest.mark.parametrize("d", [1, 7, 32, 33, 64, 128])
def test_row_widths(d, dev):
    x, y, ei = cc.random_case(150, d, 700, seed=d, spread=0.3 / np.sqrt(d))
    cc.check_against_twin(dev, x, y, ei, 5)
    cc.check_against_twin(dev, x, y, ei, 5, gamma=0, ratio=0.5, state=(d, 2))


# one edge; one short of, exactly and one past a workgroup of the classifier
@pytest.mark.parametrize("e", [1, 255, 256, 257, 1030])
def test_edge_counts(e, dev):
    x, y, ei = cc.random_case(90, 32, e, seed=e)
    if e == 1:
        ei[:] = [[3], [8]]                          # an inter edge: nodes of two runs, neither void
    (_, _, counts, _, _), _ = cc.check_against_twin(dev, x, y, ei, 5)
    if e == 1:
        assert counts.tolist() == [1, 0, 1]
    cc.check_against_twin(dev, x, y, ei, 5, ratio=0.9, state=(e, 0))


def test_hub_isolated_node_duplicate_edge(dev):
    """600 edges into node 0; node 699 without an edge (a zero row); an edge twice (it counts
    twice); two runs give the same bits."""
    n = 700
    x, y, _ = cc.random_case(n, 32, 1, seed=11)
    src = np.arange(1, 601)
    extra = np.array([[10, 10, 20, 698], [30, 30, 21, 4]])
    ei = np.concatenate([np.stack([src, np.zeros_like(src)]), extra], axis=1).astype(np.int64)
    (loss, grad, counts, _, _), want = cc.check_against_twin(dev, x, y, ei, 5)
    assert counts[2] > 400 and want["selected"][600] and want["selected"][601]
    assert not bool(grad[699].any())
    assert np.abs(want["grad"][0]).max() > 0
    (loss2, grad2, *_), _ = cc.check_against_twin(dev, x, y, ei, 5)
    assert pc.bits(loss) == pc.bits(loss2) and pc.bits(grad) == pc.bits(grad2)
    # the duplicate counts twice: without its second copy the loss differs
    keep = np.ones(ei.shape[1], dtype=bool)
    keep[601] = False
    (_, _, counts1, _, _), _ = cc.check_against_twin(dev, x, y, ei[:, keep], 5)
    assert counts1[2] == counts[2] - 1


def test_identical_rows_and_far_rows(dev):
    """d = 0: that edge's gradient is zero and finite; rows 200 apart at temperature 0.25: p
    underflows to 0 in float64, the loss stays finite."""
    x, y, ei = cc.random_case(60, 32, 200, seed=5)
    x[8] = x[9]                                     # same run of labels: an intra edge at d = 0
    x[30] += 200 / np.sqrt(32)                      # every edge at node 30 is ~200 long
    ei[:, :4] = [[8, 9, 30, 31], [9, 8, 31, 30]]
    only = ei[:, :2].copy()
    y2 = y.copy()
    y2[10, :] = 0
    y2[10, 3] = 4                                   # (an inter edge elsewhere, so the loss counts)
    for gamma in (0, 2):
        (_, grad, _, _, _), want = cc.check_against_twin(dev, x, y, ei, 5, gamma=gamma, temperature=0.25)
        assert np.isfinite(want["loss"])
        # the two rows alone, plus one inter edge between other nodes: rows 8 and 9 get exactly 0
        three = np.concatenate([only, [[10], [12]]], axis=1)
        (_, g3, c3, _, _), _ = cc.check_against_twin(dev, x, y2, three, 5, gamma=gamma, temperature=0.25)
        assert c3.tolist() == [1, 2, 3]
        assert not bool(g3[8].any()) and not bool(g3[9].any()) and bool(g3[10].any())


def test_end_out_of_range_is_dropped_and_counted(dev):
    x, y, ei = cc.random_case(90, 32, 300, seed=9)
    ei[0, 7], ei[1, 100], ei[0, 299] = -1, 90, 1 << 40
    cc.check_against_twin(dev, x, y, ei, 5, bad=3)
    cc.check_against_twin(dev, x, y, ei, 5, ratio=0.5, state=(4, 4), bad=3)


def test_strided_and_misaligned_rows_give_the_same_bits(dev):
    """A row stride larger than D (float4 loads while the stride is a multiple of 4, scalar loads
    otherwise) and a base 4 bytes off a 16-byte boundary: the bits of the dense run."""
    from superpoint_transformer_amd import ops
    x, y, ei = cc.random_case(150, 32, 700, seed=21)
    xt, yt, eit = (torch.from_numpy(a).to(dev) for a in (x, y, ei))
    loss, grad, *_ = cc.run(dev, xt, yt, eit, 5, 2, 0.8, 0.5)
    for pad, offset in ((8, 0), (5, 0), (0, 1), (3, 1)):
        flat = torch.zeros(150 * (32 + pad) + offset, device=dev)
        big = flat[offset:].view(150, 32 + pad)
        big[:, :32] = xt
        big[:, 32:] = float("nan")                  # never read
        big.requires_grad_()
        view = big[:, :32]
        assert view.stride(0) == 32 + pad and view.data_ptr() % 16 == 4 * offset
        got = ops.partition_edge_loss(view, yt, eit, 5, temperature=0.5, gamma=2, weight=0.8)
        g = torch.autograd.grad(got, big)[0]
        assert pc.bits(got) == pc.bits(loss), (pad, offset)
        assert pc.bits(g[:, :32]) == pc.bits(grad) and not bool(g[:, 32:].any())


def test_views_of_the_edge_list_are_sorted_once(dev):
    """The backward's by-source / by-target views hang on the edge_index object: the second
    backward finds them; ``csr.forget`` drops them."""
    from superpoint_transformer_amd import csr, ops
    x, y, ei = cc.random_case(150, 32, 700, seed=3)
    xt, yt, eit = (torch.from_numpy(a).to(dev) for a in (x, y, ei))
    assert not hasattr(eit, "_spt_edge_end_views")
    a = cc.run(dev, xt, yt, eit, 5)
    views = csr.edge_end_views(eit, 150)
    assert views[0].n == 700 and views[0].num_seg == 150
    b = cc.run(dev, xt, yt, eit, 5)
    assert csr.edge_end_views(eit, 150) is views and pc.bits(a[1]) == pc.bits(b[1])
    for k, v in enumerate(views):                   # stable: ascending positions inside a run
        perm, rowptr = v.perm.cpu().numpy(), v.rowptr.cpu().numpy()
        assert np.array_equal(np.sort(perm), np.arange(700))
        assert np.array_equal(ei[k][perm], np.sort(ei[k], kind="stable"))
        for s in range(150):
            assert (np.diff(perm[rowptr[s]:rowptr[s + 1]]) > 0).all()
    csr.forget(eit)
    assert not hasattr(eit, "_spt_edge_end_views")


def test_upstream_gradient_scales_the_rows(dev):
    from superpoint_transformer_amd import ops
    x, y, ei = cc.random_case(150, 32, 700, seed=8)
    xt, yt, eit = (torch.from_numpy(a).to(dev) for a in (x, y, ei))
    _, grad, *_ = cc.run(dev, xt, yt, eit, 5)
    xr = xt.clone().requires_grad_()
    (ops.partition_edge_loss(xr, yt, eit, 5) * 4).backward()
    assert pc.bits(xr.grad) == pc.bits(grad * 4)    # a power of two: exact
