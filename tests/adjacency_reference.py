"""Float64 restatement of the partition's input graph, step by step as the reference composes it:
``AdjacencyGraph(k, w)._process`` (src/transforms/graph.py:77-94), ``Data.connect_isolated``
(src/data/data.py:490-561, ``isolated_nodes`` src/utils/graph.py:44-53) and ``Data.to_trimmed``
(data.py:563-586) on ``oracle.spt_oracle.to_trimmed`` / ``coalesce`` as they are.  Plain torch on the
CPU; pinned on the reference-made fixture by tests/test_adjacency_reference_cpu.py.

Where the reference works in f32 (mean distance, weights, the lstsq fit) this works in f64; the
search for the isolated nodes' neighbours is the oracle's f32 exhaustive FRNN stand-in (squared
distances, like the search the reference calls).  A search that returns fewer than ``k_isolated``
neighbours (-1 entries) yields no edge for them - the reference would index with -1 there.
"""
import torch

from oracle import spt_oracle as O


def isolated_search(pos, is_out, k_isolated, batch=None):
    """``knn_2(pos, pos[is_out], k_isolated + 1, r_max = |bbox diagonal|)`` without column 0
    (data.py:506-517, src/utils/neighbors.py:186-242)."""
    pos = pos.float()
    r_max = (pos.max(dim=0).values - pos.min(dim=0).values).norm()
    search, query = pos, pos[is_out]
    if batch is not None:
        z_offset = pos[:, 2].max() - pos[:, 2].min() + r_max + 1
        off = torch.zeros_like(pos)
        off[:, 2] = batch * z_offset
        search, query = pos + off, (pos + off)[is_out]
    dist, idx = O.frnn_grid_points(query, search, k_isolated + 1, float(r_max))
    return idx[:, 1:], dist[:, 1:]


def partition_adjacency_reference(neighbor_index, neighbor_distance, k, w=-1, pos=None,
                                  k_isolated=1, reduce="mean", batch=None):
    """Returns a dict: ``edge_index`` [2, E] int64, ``edge_attr`` [E] f64 or None, ``source_csr``
    [N + 1], ``is_isolated`` [N] bool, ``ab`` (f64 pair or None), ``new_edge`` [E] bool (edges
    that touch an isolated node: their weights depend on the regression)."""
    if reduce not in ("mean", "add", "sum", "min", "max"):
        raise ValueError(reduce)
    nn = neighbor_index.cpu().long()
    N = nn.shape[0]
    source = torch.arange(N).repeat_interleave(k)
    target = nn[:, :k].flatten()
    mask = target >= 0
    source, target = source[mask], target[mask]
    if w > 0:
        distances = neighbor_distance.cpu()[:, :k].flatten()[mask].double()
        edge_attr = 1 / (w + distances / distances.mean())
    else:
        edge_attr = torch.ones(source.numel(), dtype=torch.float64)
    if source.numel() == 0:
        edge_attr = None
    is_isolated = torch.ones(N, dtype=torch.bool)
    is_isolated[torch.cat((source, target)).unique()] = False
    is_out = torch.where(is_isolated)[0]
    ab = None
    if k_isolated > 0 and is_out.numel() > 0:
        p = pos.cpu().float()
        nb, dist = isolated_search(p, is_out, k_isolated, None if batch is None else batch.cpu())
        new_s, new_t, dist = is_out.repeat_interleave(k_isolated), nb.flatten(), dist.flatten()
        found = new_t >= 0
        if edge_attr is not None:
            d = (p[source].double() - p[target].double()).norm(dim=1)
            d_1 = torch.vstack((d, torch.ones_like(d))).T
            a, b = torch.linalg.lstsq(d_1, edge_attr.view(-1, 1)).solution.view(-1)
            ab = (float(a), float(b))
            edge_attr = torch.cat((edge_attr, (dist.double() * a + b)[found]))
        source, target = torch.cat((source, new_s[found])), torch.cat((target, new_t[found]))
    edge_index = torch.stack((source, target))
    if edge_index.shape[1] == 0:
        edge_index, edge_attr = torch.zeros(2, 0, dtype=torch.long), None
    elif edge_attr is None:
        edge_index = O.to_trimmed(edge_index)
    else:
        edge_index, edge_attr = O.to_trimmed(edge_index, edge_attr, reduce=reduce)
    csr = torch.zeros(N + 1, dtype=torch.long)
    csr[1:] = torch.cumsum(torch.bincount(edge_index[0], minlength=N), 0)
    new_edge = is_isolated[edge_index[0]] | is_isolated[edge_index[1]]
    return dict(edge_index=edge_index, edge_attr=edge_attr, source_csr=csr,
                is_isolated=is_isolated, ab=ab, new_edge=new_edge)


REDUCE = ["mean", "add", "min", "max"]


def load_fixture_case(z, c):
    """Case ``c`` of tests/golden/adjacency.npz (indices stored as int32) as torch tensors."""
    k, w, k_iso, red = z[f"c{c}_cfg"].tolist()
    case = dict(pos=torch.from_numpy(z[f"c{c}_pos"]), nn=torch.from_numpy(z[f"c{c}_nn"]).long(),
                dist=torch.from_numpy(z[f"c{c}_dist"]), k=int(k), w=float(w), k_isolated=int(k_iso),
                reduce=REDUCE[int(red)],
                batch=torch.from_numpy(z[f"c{c}_batch"]).long() if f"c{c}_batch" in z.files else None,
                edge_index=torch.from_numpy(z[f"c{c}_edge_index"]).long(),
                edge_attr=torch.from_numpy(z[f"c{c}_edge_attr"]),
                is_isolated=torch.from_numpy(z[f"c{c}_is_isolated"]),
                ab=torch.from_numpy(z[f"c{c}_ab"]))
    return case


def relative_deviation(got, ref):
    """max |got - ref| / max |ref| (0 for empty input)."""
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp(min=1e-300))


# The weight bounds of the GPU tests.  Yardstick: the reference's own f32 result (the fixture)
# against this f64 restatement, measured on the CPU by tests/test_adjacency_reference_cpu.py
# (max |ref32 - f64| / max |f64| over an edge class, worst fixture case; the figures per case are
# in profiles/r09a_adjacency_errors.txt):
#   edges of the table (weight 1 / (w + d / mean), merged by `reduce`)           8.22e-08
#   edges of isolated nodes (a * dist + b: lstsq's f32 QR against the f64 fit)    2.76e-05
# The kernels accumulate the mean and the regression sums in f64 and get 4x these figures.
YARDSTICK_TABLE, YARDSTICK_NEW = 8.22e-08, 2.76e-05
BOUND_TABLE, BOUND_NEW = 4 * YARDSTICK_TABLE, 4 * YARDSTICK_NEW


def check_weights(got, ref, tag=""):
    """``got`` (edge_attr of the code under test) against the restatement's dict, per edge class;
    prints both deviations before asserting."""
    if ref["edge_attr"] is None:
        assert got is None, f"{tag}: edge_attr must be None when the table holds no edge"
        return 0.0, 0.0
    assert got is not None and got.dtype == torch.float32
    got, new = got.detach().cpu(), ref["new_edge"]
    dt = relative_deviation(got[~new], ref["edge_attr"][~new])
    dn = relative_deviation(got[new], ref["edge_attr"][new])
    print(f"{tag}: table edges {dt:.3e} (bound {BOUND_TABLE:.3e}), isolated-node edges {dn:.3e} "
          f"(bound {BOUND_NEW:.3e}, {int(new.sum())} edges)")
    assert dt <= BOUND_TABLE and dn <= BOUND_NEW, tag
    return dt, dn


def random_table(gen, n, K, p_missing=0.3, p_self=0.02, p_empty=0.05):
    """A synthetic ``(neighbor_index [n, K], neighbor_distance [n, K])``: every row names distinct
    nodes near its own index (so many pairs are reciprocated and many are not), in random column
    order, with entries missing at arbitrary columns, some self entries, some rows entirely
    missing and a few isolated nodes.  Row i and row j carry different distances for the same pair."""
    nn = torch.full((n, K), -1, dtype=torch.long)
    h = K // 2
    if n > 6 * K + 1:                                   # i + / - cumulated steps of 1..3: distinct, != i
        up = torch.cumsum(torch.randint(1, 4, (n, K - h), generator=gen), 1)
        down = -torch.cumsum(torch.randint(1, 4, (n, h), generator=gen), 1)
        nn = (torch.arange(n).view(-1, 1) + torch.cat((up, down), 1)) % n
        nn = torch.gather(nn, 1, torch.rand(n, K, generator=gen).argsort(1))
    elif n > 1:                                         # small: the first columns of a permutation
        kk = min(K, n - 1)
        perm = torch.rand(n, n, generator=gen).argsort(1)
        perm = perm[perm != torch.arange(n).view(-1, 1)].view(n, n - 1)
        nn[:, :kk] = perm[:, :kk]
    nn[torch.rand(n, K, generator=gen) < p_missing] = -1
    rows = torch.where(torch.rand(n, generator=gen) < p_self)[0]
    nn[rows, torch.randint(0, K, (rows.numel(),), generator=gen)] = rows
    nn[torch.rand(n, generator=gen) < p_empty] = -1
    if n >= 3:                                          # a few nodes nobody lists and that list nobody
        hermits = torch.randperm(n, generator=gen)[:min(max(n // 64, 1), 24)]
        nn[torch.isin(nn, hermits)] = -1
        nn[hermits] = -1
    dist = torch.rand(n, K, generator=gen) + 0.05
    dist[nn < 0] = -1.0
    return nn, dist
