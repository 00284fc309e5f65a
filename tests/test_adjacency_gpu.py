"""GPU parity of the partition's input graph (``graph.partition_adjacency`` on
``csrc/adjacency.hip``): kNN table in, trimmed + sorted + weighted graph with its forward star out.

Bars.  ``edge_index``, ``source_csr`` and ``num_isolated`` are EXACT: against the reference's own
output (tests/golden/adjacency.npz, made by tests/golden/make_golden_adjacency.py from the
reference's source) and against the f64 restatement tests/adjacency_reference.py on synthetic tables.
The weights have a measured bound: the reference's f32 result deviates from the f64 restatement by
8.22e-08 (table edges) and 2.76e-05 (regressed edges of isolated nodes: lstsq's f32 QR against the
f64 fit; both max |diff| / max |ref|, worst fixture case, measured on the CPU by
tests/test_adjacency_reference_cpu.py and recorded in profiles/r09a_adjacency_errors.txt); the
kernels get 4x that, 3.29e-07 and 1.10e-04.
The kernels' own figures are printed by every test before it asserts (pytest -s); they have not been
recorded on an MI355X yet.

Shapes: the table contract is on indices, so the synthetic tables need not be geometric.  N = 1, 63,
65, 257 (below / above a wave, several workgroups' worth of lane groups in the emit kernel) and
100 003 (many workgroups, odd), K = 45 with k = 10 (the strided read); a hub row of 700 foreign
entries (longer than a wave, a workgroup and any register sort); all pairs reciprocated; none."""
import pytest
import torch

import adjacency_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

_Z = None
_REF = {}


def fixture_case(c):
    global _Z
    if _Z is None:
        class Files(dict):
            files = property(lambda self: list(self))
        _Z = Files(load_golden("adjacency.npz"))
    return R.load_fixture_case(_Z, c)


def on(dev, t):
    return None if t is None else t.to(dev)


def run(dev, nn, dist, k, w=-1, pos=None, k_isolated=1, reduce="mean", batch=None):
    from superpoint_transformer_amd.graph import partition_adjacency
    return partition_adjacency(on(dev, nn), on(dev, dist), k, w=w, pos=on(dev, pos),
                               k_isolated=k_isolated, reduce=reduce, batch=on(dev, batch))


def check_graph(g, r, tag):
    assert g.edge_index.is_cuda and g.edge_index.dtype == torch.long
    assert g.source_csr.dtype == torch.long
    assert torch.equal(g.edge_index.cpu(), r["edge_index"]), tag
    assert torch.equal(g.source_csr.cpu(), r["source_csr"]), tag
    assert g.num_isolated == int(r["is_isolated"].sum()), tag
    R.check_weights(g.edge_attr, r, tag)


def check_forward_star(g, n):
    ei, csr = g.edge_index, g.source_csr
    assert csr.numel() == n + 1 and int(csr[0]) == 0 and int(csr[-1]) == ei.shape[1]
    assert torch.equal(csr[1:] - csr[:-1], torch.bincount(ei[0], minlength=n))
    if ei.shape[1] > 1:
        same = ei[0, 1:] == ei[0, :-1]
        assert bool((ei[0, 1:] >= ei[0, :-1]).all())                 # rows in order
        assert bool((ei[1, 1:] > ei[1, :-1])[same].all())            # targets increasing inside a row
    assert bool((ei[0] < ei[1]).all())


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of the sort-based route."""
    from superpoint_transformer_amd import graph
    calls = []
    inner = graph._partition_adjacency_torch

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(graph, "_partition_adjacency_torch", counted)
    return calls


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_fixture_cases_match_the_reference(c, dev, spy):
    f = fixture_case(c)
    g = run(dev, f["nn"], f["dist"], f["k"], f["w"], f["pos"], f["k_isolated"], f["reduce"], f["batch"])
    assert not spy, "the fixture's tables have no repeated neighbour: the kernels must run"
    assert torch.equal(g.edge_index.cpu(), f["edge_index"])
    assert g.num_isolated == int(f["is_isolated"].sum())
    if c not in _REF:
        _REF[c] = R.partition_adjacency_reference(f["nn"], f["dist"], f["k"], f["w"], f["pos"],
                                                  f["k_isolated"], f["reduce"], f["batch"])
    check_graph(g, _REF[c], f"fixture case {c}")
    check_forward_star(g, f["nn"].shape[0])
    # and against the reference's f32 weights themselves, at the sum of both deviations
    new = _REF[c]["new_edge"]
    got = g.edge_attr.cpu()
    assert R.relative_deviation(got[~new], f["edge_attr"][~new]) <= R.BOUND_TABLE + R.YARDSTICK_TABLE
    assert R.relative_deviation(got[new], f["edge_attr"][new]) <= R.BOUND_NEW + R.YARDSTICK_NEW


@pytest.mark.parametrize("n", [1, 63, 65, 257, 100_003])
def test_synthetic_tables_match_the_restatement(n, dev, spy):
    gen = torch.Generator().manual_seed(1000 + n)
    nn, dist = R.random_table(gen, n, 45)
    pos = torch.rand(n, 3, generator=gen) * 10
    r = R.partition_adjacency_reference(nn, dist, 10, 1.0, pos, 1, "mean")
    g = run(dev, nn, dist, 10, 1.0, pos, 1, "mean")
    assert not spy
    check_graph(g, r, f"n = {n}")
    check_forward_star(g, n)
    if n >= 63:
        assert g.num_isolated > 0 and bool((nn[:, :10] < 0).all(dim=1).any())   # the table exercises both


def hub_table(n=1024, listers=700, hub=3, K=12):
    """Row i lists i - 1 .. i - K (so no pair is mutual), the hub lists hub + 1 .. hub + K, and rows
    n - listers .. n - 1 also list the hub: its output row holds ``listers`` foreign entries."""
    i = torch.arange(n).view(-1, 1)
    nn = (i - torch.arange(1, K + 1).view(1, -1)) % n
    nn[hub] = torch.arange(hub + 1, hub + 1 + K)
    nn[n - listers:, 4] = hub
    gen = torch.Generator().manual_seed(77)
    dist = torch.rand(n, K, generator=gen) + 0.1
    return nn, dist, torch.rand(n, 3, generator=gen)


def test_hub_row_longer_than_a_workgroup(dev, spy):
    nn, dist, pos = hub_table()
    r = R.partition_adjacency_reference(nn, dist, 10, 0.5, pos, 1, "add")
    assert int(r["source_csr"][4] - r["source_csr"][3]) >= 700
    g = run(dev, nn, dist, 10, 0.5, pos, 1, "add")
    assert not spy
    check_graph(g, r, "hub")
    check_forward_star(g, nn.shape[0])


def test_hub_is_bitwise_reproducible(dev):
    nn, dist, pos = hub_table()
    a = run(dev, nn, dist, 10, 0.5, pos, 1, "mean")
    b = run(dev, nn, dist, 10, 0.5, pos, 1, "mean")
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.source_csr, b.source_csr)
    assert torch.equal(a.edge_attr.view(torch.int32), b.edge_attr.view(torch.int32))


@pytest.mark.parametrize("kind", ["all_reciprocated", "none_reciprocated"])
def test_reciprocation_extremes(kind, dev, spy):
    n, K, k = 515, 45, 10
    i = torch.arange(n).view(-1, 1)
    if kind == "all_reciprocated":                   # i +- 1..5 on a ring: every pair listed twice
        off = torch.cat((torch.arange(1, 6), -torch.arange(1, 6)))
    else:                                            # i + 1..10 on a ring of 515 > 2 k: never mutual
        off = torch.arange(1, 11)
    nn = torch.full((n, K), -1, dtype=torch.long)
    nn[:, :k] = (i + off.view(1, -1)) % n
    gen = torch.Generator().manual_seed(5)
    dist = torch.rand(n, K, generator=gen) + 0.1
    for reduce in ("mean", "max"):
        r = R.partition_adjacency_reference(nn, dist, k, 1.0, None, 1, reduce)
        g = run(dev, nn, dist, k, 1.0, None, 1, reduce)
        check_graph(g, r, f"{kind} {reduce}")
        check_forward_star(g, n)
        assert g.edge_index.shape[1] == (n * k // 2 if kind == "all_reciprocated" else n * k)
    assert not spy


def test_repeated_neighbour_takes_the_sort_route(dev, spy):
    gen = torch.Generator().manual_seed(9)
    nn, dist = R.random_table(gen, 400, 45, p_missing=0.1)
    nn[17, 2], nn[17, 7] = 30, 30                    # an oversampled neighbourhood
    dist[17, 2], dist[17, 7] = 0.4, 0.4
    nn[30, 0], nn[30, 5] = 17, 17
    dist[30, 0], dist[30, 5] = 0.2, 0.8
    pos = torch.rand(400, 3, generator=gen)
    r = R.partition_adjacency_reference(nn, dist, 10, 1.0, pos, 1, "mean")
    g = run(dev, nn, dist, 10, 1.0, pos, 1, "mean")
    assert len(spy) == 1, "a row that repeats a neighbour must go through coalesce"
    check_graph(g, r, "repeated neighbour")
    check_forward_star(g, 400)
    # the repeat outside the first k columns does not count
    nn2, dist2 = R.random_table(gen, 400, 45, p_missing=0.1)
    nn2[17, 20], nn2[17, 30] = 30, 30
    run(dev, nn2, dist2, 10, 1.0, pos, 1, "mean")
    assert len(spy) == 1


def test_all_rows_empty(dev, spy):
    nn = torch.full((5, 4), -1, dtype=torch.long)
    pos = torch.tensor([[0.0, 0, 0], [1, 0, 0], [3, 0, 0], [3, 0.5, 0], [9, 9, 9]])
    r = R.partition_adjacency_reference(nn, None, 4, -1, pos, 1)
    g = run(dev, nn, None, 4, -1, pos, 1)
    check_graph(g, r, "all rows empty")
    assert g.edge_attr is None and g.num_isolated == 5 and g.edge_index.shape[1] == r["edge_index"].shape[1] > 0
    g0 = run(dev, nn, None, 4, -1, pos, 0)
    assert tuple(g0.edge_index.shape) == (2, 0) and g0.edge_attr is None and g0.num_isolated == 5
    assert torch.equal(g0.source_csr.cpu(), torch.zeros(6, dtype=torch.long))
    assert not spy


def test_every_reduce_value(dev, spy):
    """0 <-> 1 listed by both rows at different distances, 2 -> 0 by one row only: with mean = 1 and
    w = 1 the weights are 1 / (1 + d), so every reduction gives its own number."""
    nn = torch.tensor([[1, -1, -1], [0, -1, -1], [0, -1, -1]])
    dist = torch.tensor([[0.5, -1, -1], [1.0, -1, -1], [1.5, -1, -1]])      # mean of the 3 entries: 1
    w01, w10, w20 = 1 / 1.5, 1 / 2.0, 1 / 2.5
    want = {"mean": (w01 + w10) / 2, "add": w01 + w10, "sum": w01 + w10, "min": w10, "max": w01}
    for reduce, v in want.items():
        g = run(dev, nn, dist, 3, 1.0, None, 1, reduce)
        assert g.edge_index.cpu().tolist() == [[0, 0], [1, 2]]
        assert torch.allclose(g.edge_attr.cpu().double(), torch.tensor([v, w20], dtype=torch.float64),
                              rtol=R.BOUND_TABLE, atol=0), reduce
        check_graph(g, R.partition_adjacency_reference(nn, dist, 3, 1.0, None, 1, reduce), reduce)
    assert len(set(round(v, 6) for k, v in want.items() if k != "sum")) == 4
    assert not spy
    with pytest.raises(ValueError):
        run(dev, nn, dist, 3, 1.0, None, 1, "mul")


def test_mid_size_cloud_against_the_torch_composition(dev, spy):
    """300 k voxel-lattice points + far outliers, the library's own knn_1 table at a radius that
    leaves the outliers alone; the torch composition on the device (the shims' coalesce: a sort)
    is an independent route to the same graph."""
    from superpoint_transformer_amd import graph
    from superpoint_transformer_amd.neighbors import knn_1
    from superpoint_transformer_amd.synthetic import make_voxel_cloud
    pos = make_voxel_cloud(300_000, voxel=0.03, seed=11, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    far = torch.rand(40, 3, generator=gen, device=dev) * 30 + 80
    pos = torch.cat((pos, far))[torch.randperm(pos.shape[0] + 40, generator=gen, device=dev)].contiguous()
    nn, dist = knn_1(pos, 45, r_max=0.1)
    n = pos.shape[0]
    g = graph.partition_adjacency(nn, dist, 10, w=1.0, pos=pos, k_isolated=1, reduce="mean")
    assert not spy
    ref = graph._partition_adjacency_torch(nn, dist, 10, 1.0, pos, 1, "mean", None)
    assert g.num_isolated == ref.num_isolated >= 40
    assert torch.equal(g.edge_index, ref.edge_index) and torch.equal(g.source_csr, ref.source_csr)
    touched = torch.zeros(n, dtype=torch.bool, device=dev)
    touched[nn[:, :10][nn[:, :10] >= 0]] = True
    touched |= (nn[:, :10] >= 0).any(dim=1)
    new = ~touched[g.edge_index[0]] | ~touched[g.edge_index[1]]
    dt = R.relative_deviation(g.edge_attr[~new].cpu(), ref.edge_attr[~new].cpu())
    dn = R.relative_deviation(g.edge_attr[new].cpu(), ref.edge_attr[new].cpu())
    print(f"mid size: {n} points, {g.edge_index.shape[1]} edges, {g.num_isolated} isolated; "
          f"table edges {dt:.3e}, isolated-node edges {dn:.3e}")
    assert dt <= R.BOUND_TABLE and dn <= R.BOUND_NEW
    check_forward_star(g, n)
