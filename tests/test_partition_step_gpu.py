"""The partition training stage end to end (``hotpath.SPTPartitionStep``): the graph of the
reference's chain ``KNN -> AdjacencyGraph -> RemoveKeys``, the sparse-CNN first stage,
``PartitionCriterion``, AdamW - eager and captured - and the oracle purity of ``evaluate()``.

The scene: two clouds of 612 voxels each, a floor (label 0) and a wall (label 1) meeting at an
edge, 0.1 m voxels; 7 features (position, height, a wall / floor cue with noise, noise); every
23rd voxel void."""
import functools

import numpy as np
import pytest
import torch

import partition_criterion_reference as R

pytestmark = pytest.mark.gpu

C, K, F = 2, 8, 7


@functools.lru_cache(maxsize=None)
def _scene():
    rng = np.random.default_rng(7)
    coords, label, batch = [], [], []
    for b in range(2):
        floor = np.array([(x, y, 0) for x in range(18) for y in range(18)])
        wall = np.array([(0, y, z) for y in range(18) for z in range(1, 17)])
        c = np.concatenate([floor, wall]) + (3 * b, 0, 0)
        coords.append(c)
        label.append(np.concatenate([np.zeros(len(floor)), np.ones(len(wall))]))
        batch.append(np.full(len(c), b))
    coords, label, batch = (np.concatenate(a).astype(np.int64) for a in (coords, label, batch))
    n = len(coords)
    pos = (coords * 0.1).astype(np.float32)
    cue = (label + rng.normal(size=n) * 0.5).astype(np.float32)
    x = np.concatenate([pos, pos[:, 2:], cue[:, None], rng.normal(size=(n, 2)).astype(np.float32)],
                       axis=1).astype(np.float32)
    y = np.zeros((n, C + 1), dtype=np.int64)
    y[np.arange(n), label] = rng.integers(1, 6, n)
    y[::23, :C] = 0
    y[::23, C] = 2
    assert x.shape == (1224, F)
    return pos, coords, batch, x, y


def _data(dev):
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.data import Data
    pos, coords, batch, x, y = (torch.from_numpy(a).to(dev) for a in _scene())
    d = Data(pos=pos, coords=coords, batch=batch, x=x, y=y)
    d = T.KNN(k=K, r_max=2, self_is_neighbor=False, save_as_csr=False)(d)
    d = T.AdjacencyGraph(k=K, w=0.0)(d)
    return d


def _criterion(ratio=0.9):
    from superpoint_transformer_amd.criterion import BinaryFocalLoss, PartitionCriterion
    return PartitionCriterion(BinaryFocalLoss(gamma=1), affinity_temperature=1,
                              adaptive_sampling_ratio=ratio, num_classes=C, sharding=None, seed=3)


def _step(dev, ratio=0.9):
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.hotpath import SPTPartitionStep
    d = T.RemoveKeys(keys=["edge_attr", "neighbor_index", "neighbor_distance"])(_data(dev))
    part = T.GreedyContourPriorPartition(2e-2, [5], edge_weight_mode="unit", edge_reduce="add")
    return SPTPartitionStep(d, dev, _criterion(ratio), cnn=[F, 32, 32, 32], partition=part)


def test_transforms_build_the_loss_graph(dev):
    """KNN -> AdjacencyGraph: the directed, untrimmed list (i, neighbor j of i) in row order,
    the missing neighbours left out, never across the two clouds; RemoveKeys drops the rest."""
    from superpoint_transformer_amd import transforms as T
    from superpoint_transformer_amd.neighbors import knn_1
    d = _data(dev)
    nn, dist = knn_1(d.pos, K, r_max=2, batch=d.batch)
    assert torch.equal(d.neighbor_index, nn) and torch.equal(d.neighbor_distance, dist)
    n = nn.shape[0]
    src = torch.arange(n, device=dev).repeat_interleave(K)
    keep = nn.flatten() >= 0
    assert torch.equal(d.edge_index, torch.stack([src[keep], nn.flatten()[keep]]))
    assert d.edge_index.dtype == torch.int64 and d.edge_index.shape[1] >= n * K * 0.9
    assert bool((d.batch[d.edge_index[0]] == d.batch[d.edge_index[1]]).all())
    assert not bool((d.edge_index[0] == d.edge_index[1]).any())
    assert torch.equal(d.edge_attr, torch.ones(d.edge_index.shape[1], device=dev))
    w = T.AdjacencyGraph(k=4, w=0.5)(_data(dev))
    assert w.edge_index.shape[1] <= 4 * n and w.edge_attr.shape[0] == w.edge_index.shape[1]
    flat = w.neighbor_distance[:, :4].flatten()[w.neighbor_index[:, :4].flatten() >= 0]
    assert torch.allclose(w.edge_attr, 1 / (0.5 + flat / flat.mean()))
    d = T.RemoveKeys(keys=["edge_attr", "neighbor_index", "neighbor_distance"])(d)
    assert all(d.get(k) is None for k in ("edge_attr", "neighbor_index", "neighbor_distance"))
    assert d.edge_index is not None
    with pytest.raises(Exception, match="not within Data keys"):
        T.RemoveKeys(keys="nothing_here", strict=True)(d)
    with pytest.raises(NotImplementedError, match="save_as_csr"):
        T.KNN(k=K, save_as_csr=True)
    skipped = T.KNN(k=0)(_data(dev))
    assert skipped.neighbor_index.shape[1] == K                 # (untouched)


def test_captured_replay_is_the_eager_step(dev):
    """From the same parameters and the same criterion state: 4 eager steps against one eager
    warm-up step and 3 replays - the same loss bits, the same sample sizes, the same parameters;
    the call counter advances inside the graph and the counters are device tensors."""
    eager = _step(dev)
    for g in eager.opt.param_groups:
        g["capturable"] = True                  # the AdamW arithmetic the capture sets
    le = [eager.step().detach().clone() for _ in range(4)]
    ce = eager.counts.clone()
    path = _step(dev)
    path.capture(warmup=1)
    assert path.graph is not None and path._graph_opt is True
    lc, seen = [], []
    for _ in range(3):
        lc.append(path.step().detach().clone())
        seen.append(path.counts.clone())        # a device copy: nothing is read here
    torch.cuda.synchronize(dev)
    assert [float(v) for v in le[1:]] == [float(v) for v in lc]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(le[1:], lc))
    assert path.counts.is_cuda and all(torch.equal(s, ce) for s in seen)
    assert eager.criterion.state.tolist() == path.criterion.state.tolist() == [3, 4]
    for p, q in zip(eager.params, path.params):
        assert torch.equal(p.detach(), q.detach())
    # the sample is the twin's: counts of the last call against the host rules
    d = path.data
    code, bad = R.classify(d.y.cpu().numpy(), d.edge_index.cpu().numpy(), C)
    n_inter, n_intra = int((code == 1).sum()), int((code == 2).sum())
    n_major = min(R.major_count(n_inter, 0.9), n_intra)
    assert bad == 0 and n_inter > 0 and ce.tolist() == [n_inter, n_intra, n_inter + n_major]
    assert path.criterion.status.tolist() == [0, 0]
    # successive calls drew different samples (the state advanced): the losses differ
    assert len({float(v) for v in lc}) == 3


def test_loss_falls_and_evaluate_counts_every_labelled_point(dev):
    """20 steps at the configuration's learning rate: the loss over every kept edge (eval mode: no
    sample) falls; ``evaluate()`` returns the oracle confusion matrix of the superpoints, whose
    total is the number of labelled points, and the two counts."""
    path = _step(dev)
    before, cm0, n_sp0, n_p0 = path.evaluate()
    for _ in range(20):
        loss = path.step()
    assert bool(torch.isfinite(loss))
    after, cm, n_sp, n_p = path.evaluate()
    print(f"eval loss {float(before):.6f} -> {float(after):.6f}; superpoints {n_sp0} -> {n_sp} of {n_p}")
    assert float(after) < float(before)
    y = path.data.y
    for m in (cm0, cm):
        assert int(m.confmat.sum()) == int(y[:, :C].sum())
        assert 0 < m.oa() <= 100
    assert n_p == n_p0 == y.shape[0] and 1 <= n_sp < n_p and 1 <= n_sp0 < n_p
    # the oracle labels every superpoint with its majority: off the diagonal only mixed superpoints
    assert cm.confmat.diag().sum() >= cm.confmat.sum() - cm.confmat.diag().sum()
    with pytest.raises(ValueError, match="partition transform"):
        type(path)(path.data, dev, _criterion()).evaluate()
    with pytest.raises(ValueError, match="PartitionCriterion"):
        type(path)(path.data, dev, torch.nn.CrossEntropyLoss())
