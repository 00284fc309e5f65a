"""CPU suite of the greedy contour-prior partition: the package's torch composition (the route of
CPU tensors) against the host twin, exactly, and the invariants of the result."""
import numpy as np
import pytest
import torch

import greedy_partition_reference as R
from superpoint_transformer_amd import partition as P
from superpoint_transformer_amd.data import Data


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


_bits, assert_same = R.bits, R.assert_same


def run_both(x, pos, ei, w, reg, min_size, device="cpu", **kw):
    S = np.ones(x.shape[0], dtype=np.int64)
    want = R.merge(x, S, ei, w, reg, min_size, P=pos, **kw)
    got = P.merge_components_by_contour_prior(
        _t(x).to(device), _t(S).to(device), _t(ei).to(device), None if w is None else _t(w).to(device),
        reg, min_size, P=_t(pos).to(device), **kw)
    return got, want


@pytest.fixture(scope="module")
def grid24():
    return R.grid_case(24, 0.3, D=2, seed=1)


@pytest.mark.parametrize("D", [1, 7])
def test_cpu_route_equals_twin_on_grid(D):
    x, pos, ei = R.grid_case(16, 0.3, D=D, seed=D)
    got, want = run_both(x, pos, ei, None, 2e-2, 5)
    assert want[1] >= 2                                   # several rounds, real merges
    assert_same(got, want)


@pytest.mark.parametrize("reduce", ["add", "mean", "max", "min", "mul"])
def test_cpu_component_graph_every_reduce(reduce):
    rng = np.random.default_rng(3)
    ei = rng.integers(0, 12, size=(2, 300)).astype(np.int64)       # duplicates, loops, both ways
    w = rng.uniform(0.5, 1.5, 300).astype(np.float32)
    index = rng.integers(0, 5, size=12).astype(np.int64)
    index[:5] = np.arange(5)
    for idx in (None, index):
        wE, wW = R.component_graph(idx, ei, w, reduce)
        gE, gW = P.component_graph(None if idx is None else _t(idx), _t(ei), _t(w), reduce,
                                   num_components=12 if idx is None else 5)
        assert np.array_equal(gE.numpy(), wE)
        assert np.array_equal(_bits(gW), _bits(wW))


def test_cpu_long_runs_take_the_strided_sums():
    """A pair listed 600 times and a star that merges 600 leaves into its hub in one round: both
    summation rules beyond 512 members."""
    n = 601
    ei = np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n, dtype=np.int64)])
    ei = np.concatenate([ei, np.tile(np.array([[1], [2]]), (1, 600))], 1)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    pos = rng.standard_normal((n, 3)).astype(np.float32)
    trace = []
    S = np.ones(n, dtype=np.int64)
    want = R.merge(x, S, ei, w, 2e-2, 5, P=pos, trace=trace)
    assert trace[0]["largest"] > R.LONG_RUN
    got = P.merge_components_by_contour_prior(_t(x), _t(S), _t(ei), _t(w), 2e-2, 5, P=_t(pos))
    assert_same(got, want)
    for reduce in ("add", "mean", "max", "mul"):
        wE, wW = R.component_graph(None, ei, w, reduce)
        gE, gW = P.component_graph(None, _t(ei), _t(w), reduce, num_components=n)
        assert np.array_equal(gE.numpy(), wE) and np.array_equal(_bits(gW), _bits(wW))


def test_cpu_options_equal_twin(grid24):
    x, pos, ei = grid24
    for kw in (dict(merge_only_small=True), dict(max_iterations=1), dict(reduce="max")):
        got, want = run_both(x, pos, ei, None, 2e-2, 5, **kw)
        assert_same(got, want)
    assert run_both(x, pos, ei, None, 2e-2, 5, max_iterations=1)[1][1] == 1


def _union_find_components(n, ei, keep):
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(ei[0][keep], ei[1][keep]):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(a) for a in range(n)])


def test_invariants_of_an_unbounded_run(grid24):
    x, pos, ei = grid24
    N = x.shape[0]
    reg, min_size = 2e-2, 5
    I, _, (X, S, E, W, Pm) = P.merge_components_by_contour_prior(
        _t(x), torch.ones(N, dtype=torch.int64), _t(ei), None, reg, min_size, P=_t(pos))
    I, X, S, E, W, Pm = (t.numpy() for t in (I, X, S, E, W, Pm))
    assert S.sum() == N and np.array_equal(np.bincount(I), S)
    # every component is connected in the input graph: the edges inside components span them
    inside = I[ei[0]] == I[ei[1]]
    cc = _union_find_components(N, ei, inside)
    assert len(np.unique(cc)) == len(S)
    assert all(len(np.unique(I[cc == c])) == 1 for c in np.unique(cc))
    # the quotient of the input graph under the final labels, computed directly (unit weights:
    # every f32 sum is an integer, so the order of the sums does not matter)
    qE, qW = R.quotient(I, ei, None, "add")
    assert np.array_equal(E, qE) and np.array_equal(_bits(W), _bits(qW))
    # nothing is left to do: no small component with an edge, no edge with a negative gain
    F = np.stack([x[I == c].astype(np.float64).sum(0) for c in range(len(S))])
    has_edge = np.zeros(len(S), dtype=bool)
    has_edge[E.ravel()] = True
    assert not (has_edge & (S < min_size)).any()
    assert not (R.gains(F, S, E, W, reg) < 0).any()
    # means within 1 ulp of f32 of an f64 recomputation from the labels: two f64 summation orders
    # can move an f32 rounding by one step, and by no more
    for got, src in ((X, x), (Pm, pos)):
        ref = np.stack([src[I == c].astype(np.float64).mean(0) for c in range(len(S))]).astype(np.float32)
        assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()


def test_cpu_on_data_with_and_without_super_index(grid24):
    x, pos, ei = grid24
    N = x.shape[0]
    rng = np.random.default_rng(2)
    sizes = rng.integers(1, 4, N).astype(np.int64)
    start = (np.arange(N) // 3).astype(np.int64)                   # triples along the rows
    w = np.ones(ei.shape[1], dtype=np.float32)
    for si in (None, start):
        data = Data(x=_t(x), pos=_t(pos), edge_index=_t(ei), edge_attr=_t(w), node_size=_t(sizes))
        if si is not None:
            data.super_index = _t(si)
        out, (X, S, E, W, Pm, sub) = P.merge_components_by_contour_prior_on_data(data, 2e-2, 30)
        wI, _, (wX, wS, wE, wW, wP) = R.merge_on_data(x, pos, ei, w, 2e-2, 30, super_index=si,
                                                      node_size=sizes)
        assert np.array_equal(out.super_index.numpy(), wI)
        assert np.array_equal(S.numpy(), wS) and np.array_equal(E.numpy(), wE)
        for g, t in ((X, wX), (W, wW), (Pm, wP)):
            assert np.array_equal(_bits(g), _bits(t))
        assert data.get("super_index") is None or si is not None    # the input keeps its own
        # sub: the members of every component, ascending
        assert sub.num_clusters == len(wS) and sub.ascending
        assert np.array_equal(sub.to_super_index().numpy(), wI)


def test_cpu_edge_weights_and_refusals(grid24):
    x, pos, ei = grid24
    dist, total = P.edge_lengths(_t(pos), _t(ei))
    want = R.edge_lengths(pos, ei)
    assert np.array_equal(_bits(dist), _bits(want))
    assert abs(total - want.astype(np.float64).sum()) <= 1e-12 * total
    assert torch.equal(P.edge_weights(_t(pos), _t(x), _t(ei), "unit"), torch.ones(ei.shape[1]))
    for mode, rows in (("inverse_distance", pos), ("exp_neg_distance", pos),
                       ("exp_neg_latent_distance", x)):
        got = P.edge_weights(_t(pos), _t(x), _t(ei), mode, d_0=0.75).numpy()
        ref = R.weights_from_lengths(R.edge_lengths(rows, ei), mode, 0.75)
        # the division is IEEE on both sides; exp may differ by the libraries' last bits
        assert (np.abs(got - ref) <= (0 if mode == "inverse_distance" else 2) * np.spacing(ref)).all()
    with pytest.raises(NotImplementedError):
        P.edge_weights(_t(pos), _t(x), _t(ei), "affinity_latent_distance")
    with pytest.raises(ValueError):
        P.edge_weights(_t(pos), _t(x), _t(ei), "affinity_latent_distance_exp_neg")
    with pytest.raises(NotImplementedError):
        P.merge_components_by_contour_prior(_t(x), torch.ones(len(x), dtype=torch.int64), _t(ei),
                                            None, 2e-2, 5, k=3)
    with pytest.raises(ValueError):
        P.merge_components_by_contour_prior(_t(x), torch.full((len(x),), 1 << 29), _t(ei), None,
                                            2e-2, 5)
    with pytest.raises(ValueError):
        P.component_graph(None, _t(ei), None, "median", num_components=len(x))


def test_twin_meets_min_size_and_keeps_the_plateaus_apart():
    """The specification behaves: at low noise the result meets min_size and no component mixes
    two plateaus.  (Round counts are whatever they are: the tests compare with the twin, never
    with constants.)"""
    n = 16
    x, pos, ei = R.grid_case(n, 0.05, D=2, seed=4)
    I, it, (X, S, E, W, _) = R.merge(x, np.ones(n * n, dtype=np.int64), ei, None, 2e-2, 5)
    assert it >= 1 and (S >= 5).all()
    plateau = (np.arange(n * n) // n >= n // 2) * 2 + (np.arange(n * n) % n >= n // 2)
    assert all(len(np.unique(plateau[I == c])) == 1 for c in range(len(S)))
