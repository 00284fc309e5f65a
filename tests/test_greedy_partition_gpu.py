"""The greedy contour-prior partition on the device (csrc/merge.hip) against the host twin
(tests/greedy_partition_reference.py): labels, round count, sizes, graph, weights and means bit
for bit."""
import numpy as np
import pytest
import torch

import greedy_partition_reference as R

pytestmark = pytest.mark.gpu

REG = 2e-2


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def both(dev, x, pos, ei, w, min_size, sizes=None, **kw):
    from superpoint_transformer_amd import partition as P
    S = np.ones(np.asarray(x).shape[0], dtype=np.int64) if sizes is None else sizes
    want = R.merge(x, S, ei, w, REG, min_size, P=pos, **kw)
    got = P.merge_components_by_contour_prior(_t(x, dev), _t(S, dev), _t(ei, dev), _t(w, dev), REG,
                                              min_size, P=_t(pos, dev), **kw)
    assert all(t is None or t.is_cuda for t in (got[0],) + tuple(got[2]))
    R.assert_same(got, want)
    return got, want


def _edges(pairs):
    return np.array(pairs, dtype=np.int64).reshape(-1, 2).T.copy()


TINY = {
    "one node": (1, []),
    "two nodes, one edge": (2, [(0, 1)]),
    "no edges": (5, []),
    "only self loops": (4, [(0, 0), (2, 2), (2, 2), (3, 3)]),
    "a node with no edge among connected ones": (7, [(0, 1), (1, 0), (1, 2), (4, 5), (5, 6), (6, 4),
                                                     (2, 2)]),
}


@pytest.mark.parametrize("name", sorted(TINY))
def test_tiny_graphs(name, dev):
    n, pairs = TINY[name]
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    pos = rng.standard_normal((n, 3)).astype(np.float32)
    (I, it, (X, S, E, W, Pm)), want = both(dev, x, pos, _edges(pairs), None, 3)
    assert I.shape == (n,) and E.shape[0] == 2 and W.shape == (E.shape[1],)
    if name == "a node with no edge among connected ones":
        assert want[1] >= 1 and int(S[I[3]]) == 1                   # it stays alone


@pytest.mark.parametrize("D", [1, 7, 33])
def test_grid_24_with_noise(D, dev):
    x, pos, ei = R.grid_case(24, 0.3, D=D, seed=D)
    _, want = both(dev, x, pos, ei, None, 5)
    assert want[1] >= 3


def test_grid_48_without_noise_long_sums_and_deep_chains(dev):
    """Ties everywhere: one round, trees of 576 > 512 members (the strided sums) and the deepest
    pointer chains."""
    x, pos, ei = R.grid_case(48, 0.0, D=2, seed=0)
    trace = []
    R.merge(x, np.ones(48 * 48, dtype=np.int64), ei, None, REG, 5, trace=trace)
    assert trace[0]["largest"] > R.LONG_RUN and trace[0]["passes"] >= 4
    both(dev, x, pos, ei, None, 5)


def _duplicated(seed=3, n=40, e=900):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, size=(2, e)).astype(np.int64)          # duplicates, loops, both ways
    ei[:, -560:] = np.array([[1], [0]])                             # one pair 560 times: a long run
    w = rng.uniform(0.5, 1.5, e).astype(np.float32)
    return n, ei, w


@pytest.mark.parametrize("reduce", ["add", "mean", "max", "min", "mul"])
def test_every_reduce_on_duplicates(reduce, dev):
    from superpoint_transformer_amd import partition as P
    n, ei, w = _duplicated()
    index = np.random.default_rng(1).integers(0, 9, n).astype(np.int64)
    index[:9] = np.arange(9)
    for idx, C in ((None, n), (index, 9)):
        wE, wW = R.component_graph(idx, ei, w, reduce)
        gE, gW = P.component_graph(_t(idx, dev), _t(ei, dev), _t(w, dev), reduce, num_components=C)
        assert np.array_equal(R.bits(gE), wE) and np.array_equal(R.bits(gW), R.bits(wW))
    rng = np.random.default_rng(4)
    x = rng.standard_normal((n, 4)).astype(np.float32)
    pos = rng.standard_normal((n, 3)).astype(np.float32)
    both(dev, x, pos, ei, w, 4, reduce=reduce)


@pytest.mark.parametrize("E,loops", [(4095, 37), (4096, 5), (4097, 1)])
def test_component_graph_at_the_sort_tile_seam(E, loops, dev):
    """E around the 4096 keys of one sort tile, 50 components under a relabelling of 200 nodes:
    duplicates in both directions, and `loops` edges that the relabelling turns into self loops -
    the rejected tail of the sorted keys, which starts at position 4096 for E = 4097.  Against
    the package's CPU route, every reduce, bit for bit (both reduce a run in input order)."""
    from superpoint_transformer_amd import partition as P
    rng = np.random.default_rng(E)
    C, n = 50, 200
    index = (np.arange(n) % C).astype(np.int64)
    a = rng.integers(0, C, E)
    b = (a + rng.integers(1, C, E)) % C                              # another component
    b[:loops] = a[:loops]                                            # the same one: dropped
    ei = np.stack([a + C * rng.integers(0, n // C, E), b + C * rng.integers(0, n // C, E)])
    ei = ei[:, rng.permutation(E)].astype(np.int64)
    w = rng.uniform(0.5, 1.5, E).astype(np.float32)
    kept = int((index[ei[0]] != index[ei[1]]).sum())
    assert kept == E - loops and 0 < loops
    for reduce in ("add", "mean", "max", "min", "mul"):
        wE, wW = P.component_graph(_t(index, "cpu"), _t(ei, "cpu"), _t(w, "cpu"), reduce,
                                   num_components=C)
        gE, gW = P.component_graph(_t(index, dev), _t(ei, dev), _t(w, dev), reduce, num_components=C)
        assert gE.is_cuda and wE.shape[1] < kept                     # duplicates were merged
        assert torch.equal(gE.cpu(), wE), reduce
        assert torch.equal(gW.cpu().view(torch.int32), wW.view(torch.int32)), reduce


def test_merge_only_small_and_one_iteration(dev):
    x, pos, ei = R.grid_case(24, 0.3, D=2, seed=1)
    both(dev, x, pos, ei, None, 5, merge_only_small=True)
    _, want = both(dev, x, pos, ei, None, 5, max_iterations=1)
    assert want[1] == 1


def _data(dev, x, pos, ei, w, **more):
    from superpoint_transformer_amd.data import Data
    return Data(x=_t(x, dev), pos=_t(pos, dev), edge_index=_t(ei, dev), edge_attr=_t(w, dev),
                **{k: _t(v, dev) for k, v in more.items()})


def test_on_data_from_a_given_super_index(dev):
    from superpoint_transformer_amd import partition as P
    x, pos, ei = R.grid_case(24, 0.3, D=2, seed=1)
    N = x.shape[0]
    sizes = np.random.default_rng(2).integers(1, 4, N).astype(np.int64)
    start = (np.arange(N) // 3).astype(np.int64)
    w = np.ones(ei.shape[1], dtype=np.float32)
    for si in (None, start):
        more = dict(node_size=sizes) if si is None else dict(node_size=sizes, super_index=si)
        out, (X, S, E, W, Pm, sub) = P.merge_components_by_contour_prior_on_data(
            _data(dev, x, pos, ei, w, **more), REG, 30)
        wI, it, rest = R.merge_on_data(x, pos, ei, w, REG, 30, super_index=si, node_size=sizes)
        R.assert_same((out.super_index, it, (X, S, E, W, Pm)), (wI, it, rest))
        assert sub.ascending and np.array_equal(R.bits(sub.to_super_index()), wI)


@pytest.mark.parametrize("mode", ["inverse_distance", "exp_neg_distance", "exp_neg_latent_distance"])
def test_distance_weight_modes(mode, dev):
    """The edge lengths are the twin's bits.  The elementwise part (two divisions, or a division
    and an exp) runs in torch's own device kernels, which promise no more than a last-bit error
    per operation: the weights are compared within 2 ulp and the merge runs on the package's
    weights on both sides."""
    from superpoint_transformer_amd import partition as P
    x, pos, ei = R.grid_case(24, 0.3, D=7, seed=7)
    rows = x if mode == "exp_neg_latent_distance" else pos
    dist, total = P.edge_lengths(_t(rows, dev), _t(ei, dev))
    want = R.edge_lengths(rows, ei)
    assert np.array_equal(R.bits(dist), R.bits(want))
    exact = want.astype(np.float64).sum()
    assert abs(total - exact) <= 1e-12 * exact
    slack = 2
    for d_0 in (0.75, None):
        got = P.edge_weights(_t(pos, dev), _t(x, dev), _t(ei, dev), mode, d_0=d_0)
        ref = R.weights_from_lengths(want, mode, np.float32(total / ei.shape[1]) if d_0 is None else d_0)
        assert (np.abs(got.cpu().numpy() - ref) <= slack * np.spacing(ref)).all()
    both(dev, x, pos, ei, got.cpu().numpy(), 5)


def test_transform_three_levels(dev):
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.csr import adopt_csr
    x, pos, ei = R.grid_case(48, 0.3, D=2, seed=5)
    N = x.shape[0]
    y = np.zeros((N, 4), dtype=np.int64)
    y[np.arange(N), np.random.default_rng(0).integers(0, 4, N)] = 1
    min_size = [5, 30, 90]
    nag = T.GreedyContourPriorPartition(REG, min_size)(_data(dev, x, pos, ei, None, y=y))
    assert nag.num_levels == 4
    # against the twin, level by level ('unit' resets the weights at every level)
    lx, lp, le, ls = x, pos, ei, None
    for lvl, ms in enumerate(min_size):
        wI, _, (wX, wS, wE, wW, wP) = R.merge_on_data(lx, lp, le, None, REG, ms, node_size=ls)
        up = nag[lvl + 1]
        assert np.array_equal(R.bits(nag[lvl].super_index), wI)
        # as in the reference the next level overwrites a level's merged weights with the mode's
        top = lvl == len(min_size) - 1
        for g, t in ((up.x, wX), (up.pos, wP), (up.node_size, wS), (up.edge_index, wE),
                     (up.edge_attr, wW if top else np.ones_like(wW))):
            assert np.array_equal(R.bits(g), R.bits(t))
        assert (wS >= ms).all() or wE.shape[1] == 0
        lx, lp, le, ls = wX, wP, wE, wS
    for lvl in range(1, 4):
        up, si = nag[lvl], nag[lvl - 1].super_index
        n_up = up.num_nodes
        assert int(si.max()) + 1 == n_up                                    # levels nested
        assert adopt_csr(si, n_up, up.sub.pointers, up.sub.points, verify="now") is not None
        assert torch.equal(up.y.sum(0), _t(y, dev).sum(0)) and up.y.dtype == torch.int64
        assert int(up.node_size.sum()) == N
    # the NAG is one the later transforms take
    nag = T.SegmentFeatures(n_max=16, n_min=4, mean_keys=[], std_keys=[])(nag)
    nag = T.RadiusHorizontalGraph(k_min=1, k_max=8, gap=2.0)(nag)
    for lvl in range(1, 4):
        assert nag[lvl].edge_index.shape[0] == 2


def test_transform_spatial_weight_widens_x(dev):
    from superpoint_transformer_amd import transforms as T
    x, pos, ei = R.grid_case(24, 0.3, D=2, seed=6)
    nag = T.GreedyContourPriorPartition([REG, REG], [5, 30], spatial_weight=0.1,
                                        edge_weight_mode="exp_neg_distance", edge_reduce="mean")(
        _data(dev, x, pos, ei, None))
    assert [nag[i].x.shape[1] for i in range(3)] == [5, 8, 8]
    assert torch.equal(nag[0].x[:, 2:], nag[0].pos * 0.1)


def test_refusals(dev):
    from superpoint_transformer_amd import partition as P, transforms as T
    with pytest.raises(NotImplementedError, match="k > 0"):
        T.GreedyContourPriorPartition(REG, 5, k=2)
    with pytest.raises(NotImplementedError, match="epsilon_edge_weight"):
        T.GreedyContourPriorPartition(REG, 5, edge_weight_mode="affinity_latent_distance")
    with pytest.raises(ValueError, match="raises"):
        T.GreedyContourPriorPartition(REG, 5, edge_weight_mode="affinity_latent_distance_exp_neg")
    with pytest.raises(AssertionError):
        T.GreedyContourPriorPartition(REG, 5, edge_weight_mode="nearest")
    with pytest.raises(AssertionError):
        T.GreedyContourPriorPartition([REG], [5, 30])
    x, pos, ei = R.grid_case(4, 0.3)
    with pytest.raises(ValueError, match="2\\^29"):
        P.merge_components_by_contour_prior(_t(x, dev), torch.full((16,), 1 << 29, device=dev),
                                            _t(ei, dev), None, REG, 5)
    bad = ei.copy()
    bad[1, 3] = 16
    with pytest.raises(ValueError, match="out of range"):
        P.component_graph(None, _t(bad, dev), None, "add", num_components=16)
    with pytest.raises(ValueError, match="out of range"):
        P.edge_lengths(_t(pos, dev), _t(bad, dev))
