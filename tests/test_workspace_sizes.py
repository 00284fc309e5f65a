"""CPU suite: the workspaces of the six entries that sort wide keys and find runs
(csrc/sorted_runs.hpp) are no larger than they were before the entries shared that helper.

The queries are host-only arithmetic, so the margin is zero.  PARENT holds what the library of
commit 0cc0820 (the last one with a private plan in each of voxel.hip, panoptic.hip,
sparse_conv.hip, merge.hip and cluster_graph.hip) answered for the same arguments."""
import pytest

N = (1, 4096, 4097, 1_000_003)          # around SORT_TILE = 4096, and a size no tile divides
BITS = (1, 32, 33, 63)                  # one word, its last width, two words, the widest key

# entry -> n -> bytes per key width of BITS (one value where the entry takes no width)
PARENT = {  # commit 0cc0820
    "spt_voxel_groups_workspace_bytes": {
        1: (3328, 3328, 4096, 4096),
        4096: (116480, 116480, 165632, 165632),
        4097: (119040, 119040, 168960, 168960),
        1_000_003: (28253952, 28253952, 40254720, 40254720)},
    "spt_merge_instances_workspace_bytes": {
        1: (3840, 3840, 4608, 4608),
        4096: (149504, 149504, 198656, 198656),
        4097: (152320, 152320, 202240, 202240),
        1_000_003: (36254464, 36254464, 48255232, 48255232)},
    "spt_pair_stats_workspace_bytes": {        # (P, G = P, bits)
        1: (4352, 4352, 5120, 5120),
        4096: (215040, 215040, 264192, 264192),
        4097: (218368, 218368, 268288, 268288),
        1_000_003: (52254976, 52254976, 64255744, 64255744)},
    "spt_sparse_map_count_workspace_bytes": {
        1: (3072, 3072, 3840, 3840),
        4096: (99840, 99840, 148992, 148992),
        4097: (102400, 102400, 152320, 152320),
        1_000_003: (24253696, 24253696, 36254464, 36254464)},
    "spt_component_graph_workspace_bytes": {   # (E)
        1: (4096,), 4096: (165888,), 4097: (168960,), 1_000_003: (40254720,)},
    "spt_cluster_graph_edges_workspace_bytes": {   # (S = n, k = 1)
        1: (3584,), 4096: (134912,), 4097: (135680,), 1_000_003: (32254208,)},
}


def _ask(L, name, n):
    fn = getattr(L, name)
    if name == "spt_pair_stats_workspace_bytes":
        return tuple(fn(n, n, b) for b in BITS)
    if name == "spt_component_graph_workspace_bytes":
        return (fn(n),)
    if name == "spt_cluster_graph_edges_workspace_bytes":
        return (fn(n, 1),)
    return tuple(fn(n, b) for b in BITS)


@pytest.mark.parametrize("name", sorted(PARENT))
def test_workspace_is_no_larger_than_the_parents(name):
    from superpoint_transformer_amd import _lib
    for n in N:
        got, was = _ask(_lib.lib, name, n), PARENT[name][n]
        print(f"{name} n={n}: {got} (parent {was})")
        assert len(got) == len(was)
        for g, w in zip(got, was):
            assert 0 < g <= w, f"{name} n={n}: {got} bytes, the parent asked for {was}"
