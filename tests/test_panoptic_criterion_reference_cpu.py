"""The CPU route of the panoptic criterion - ``panoptic.major_objects``, ``ops.edge_affinity_loss``,
``criterion.EdgeAffinityCriterion`` / ``PanopticCriterion``, ``metrics.BinaryEdgeStats`` on CPU
tensors - against tests/golden/panoptic_criterion.npz, the reference's own output
(tests/panoptic_criterion_cases.py holds the comparisons; the device runs the same ones in
tests/test_panoptic_criterion_gpu.py)."""
import panoptic_criterion_cases as cc

CPU = "cpu"


def test_major_objects_equal_the_reference():
    cc.check_major(CPU)


def test_a_cluster_without_a_pair_is_refused():
    cc.check_empty_cluster(CPU)


def test_void_masks_and_edge_cases_are_exact():
    cc.check_masks_and_cases(CPU)


def test_losses_gradients_and_counters_in_every_setting():
    cc.check_losses(CPU)


def test_criterion_on_an_output_object():
    cc.check_output_route(CPU)


def test_combined_loss_of_model_step():
    cc.check_combined(CPU)


def test_all_void_edges_give_nan_and_a_zero_gradient():
    cc.check_all_void(CPU)


def test_no_edge_at_all():
    cc.check_no_edge(CPU)


def test_extreme_logits_stay_finite():
    cc.check_extreme_logits(CPU)


def test_binary_edge_stats():
    cc.check_metric(CPU)
