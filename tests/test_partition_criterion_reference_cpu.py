"""The float64 host twin (tests/partition_criterion_reference.py) and the CPU route of the
partition criterion - ``ops.partition_edge_loss``, ``criterion.PartitionCriterion`` /
``BinaryFocalLoss``, ``output.PartitionOutput`` on CPU tensors - against
tests/golden/partition_criterion.npz, the reference's own output (tests/partition_criterion_cases.py
holds the comparisons; the device runs the same ones in tests/test_partition_criterion_gpu.py)."""
import numpy as np
import pytest
import torch

import partition_criterion_cases as cc
import partition_criterion_reference as R
from augment_reference import rand32, rand32_scalar

CPU = "cpu"


def test_twin_equals_the_reference_in_float64():
    cc.check_twin_against_fixture()


def test_losses_gradients_and_counters_in_every_setting():
    cc.check_fixture(CPU)


def test_all_void_and_single_label_give_exactly_zero():
    cc.check_fake_losses(CPU)


def test_label_vector_decides_like_the_histograms():
    cc.check_label_vector(CPU)


@pytest.mark.parametrize("ratio", cc.RATIOS)
def test_sample_equals_the_twins(ratio):
    cc.check_sampling(CPU, ratio)


def test_criterion_on_a_partition_output():
    cc.check_criterion(CPU)


def test_arguments_are_refused():
    cc.check_arguments(CPU)


def test_generator_of_the_cpu_route_is_the_kernels():
    """The torch restatement of ``rand32`` (int64 products that wrap, masked shifts) and the
    call-seed mix against the integer forms."""
    from superpoint_transformer_amd import ops
    for seed in (0, 1234, (1 << 64) - 3, 0x9E3779B97F4A7C15):
        got = ops._rand32_torch(seed, 500, "cpu").numpy().astype(np.uint64)
        assert np.array_equal(got, rand32(seed, np.arange(500)))
        assert int(got[7]) == rand32_scalar(seed, 7) == ops._rand32_int(seed, 7)
    for seed, calls in ((0, 0), (77, 3), (-5, 1 << 40)):
        assert ops.partition_call_seed(seed, calls) == R.call_seed(seed, calls)
    assert R.call_seed(0, 0) != R.call_seed(0, 1)


def test_major_count_is_torchs_arithmetic():
    """``((1 / r - 1) * count).int()`` of the reference against the twin's f32 product."""
    for ratio in (0.9, 0.5, 0.1, 0.3, 0.75):
        for count in (0, 1, 9, 220, 12345, 1_000_003, 8_999_999):
            want = int(((1 / ratio - 1) * torch.tensor(count).int().sum()).int())
            assert R.major_count(count, ratio) == want, (ratio, count)


def test_gradient_of_the_twin_by_finite_differences():
    """Central differences of the twin's loss on 5 rows (float64: the step error is ~1e-9 of the
    gradient's scale)."""
    g = cc.golden()
    args = (g["y"], g["edge_index"], int(g["num_classes"]), 0.25, 2, 0.8)
    base = R.loss_and_grad(g["x"], *args)
    x = g["x"].astype(np.float64)
    scale = np.abs(base["grad"]).max()
    h = 1e-6
    for row in (1, 77, 150, 222, 299):             # (not 40 / 41: at distance 0 the norm has a kink)
        assert np.abs(base["grad"][row]).max() > 0
        for col in (0, 13, 31):
            xp, xm = x.copy(), x.copy()
            xp[row, col] += h
            xm[row, col] -= h
            fd = (R.loss_and_grad(xp, *args)["loss"] - R.loss_and_grad(xm, *args)["loss"]) / (2 * h)
            assert abs(fd - base["grad"][row, col]) <= 1e-6 * scale, (row, col)
    # rows 40 and 41 hold the same point and are joined: that edge adds nothing to either row
    e, d, _, c = R.edge_terms(g["x"], g["edge_index"], base["selected"], base["code"], 0.25, 2, 0.8, 1e-6)
    zero = d == 0
    assert zero.sum() >= 2 and not c[zero].any() and np.isfinite(base["grad"]).all()
