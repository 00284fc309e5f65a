"""``transforms.AdjacencyGraph`` / ``RemoveKeys`` / ``KNN``'s refusals and ``output.PartitionOutput``
on CPU tensors (the search itself runs on the device: tests/test_partition_step_gpu.py)."""
import pytest
import torch


def _data():
    from superpoint_transformer_amd.data import Data
    nn = torch.tensor([[1, 2, -1], [0, 2, 3], [1, -1, -1], [2, 1, 0]])
    dist = torch.tensor([[1.0, 2.0, -1.0], [1.0, 1.5, 3.0], [1.5, -1.0, -1.0], [0.5, 3.0, 4.0]])
    return Data(pos=torch.zeros(4, 3), neighbor_index=nn, neighbor_distance=dist)


def test_adjacency_graph_is_the_directed_untrimmed_list():
    from superpoint_transformer_amd import transforms as T
    d = T.AdjacencyGraph(k=2, w=0.0)(_data())
    assert d.edge_index.tolist() == [[0, 0, 1, 1, 2, 3, 3], [1, 2, 0, 2, 1, 2, 1]]
    assert d.edge_attr.tolist() == [1.0] * 7 and d.edge_attr.dtype == torch.float32
    d = T.AdjacencyGraph(k=3, w=0.5)(_data())
    assert d.edge_index.shape == (2, 9)
    flat = torch.tensor([1.0, 2.0, 1.0, 1.5, 3.0, 1.5, 0.5, 3.0, 4.0])
    assert torch.allclose(d.edge_attr, 1 / (0.5 + flat / flat.mean()))
    with pytest.raises(AssertionError):
        T.AdjacencyGraph(k=4)(_data())
    from superpoint_transformer_amd.data import Data
    with pytest.raises(AssertionError, match="neighbor_index"):
        T.AdjacencyGraph(k=1)(Data(pos=torch.zeros(2, 3)))


def test_remove_keys_and_knn_refusals():
    from superpoint_transformer_amd import transforms as T
    d = T.AdjacencyGraph(k=2, w=0.0)(_data())
    d = T.RemoveKeys(keys=["edge_attr", "neighbor_index", "neighbor_distance"])(d)
    assert d.get("edge_attr") is None and d.get("neighbor_index") is None
    assert d.edge_index is not None and d.pos is not None
    assert T.RemoveKeys(keys="not_there")(d) is d
    with pytest.raises(Exception, match="not within Data keys"):
        T.RemoveKeys(keys="not_there", strict=True)(d)
    with pytest.raises(NotImplementedError, match="save_as_csr"):
        T.KNN(k=8, save_as_csr=True)
    same = _data()
    assert T.KNN(k=8, r_max=0)(same) is same and T.KNN(k=0)(same) is same


def test_partition_output():
    from superpoint_transformer_amd.data import Cluster, Data
    from superpoint_transformer_amd.output import PartitionOutput
    y = torch.tensor([[1, 0, 0], [0, 2, 1]])
    out = PartitionOutput(y, torch.zeros(2, 4), torch.zeros(2, 0, dtype=torch.long), extra=5)
    assert out.has_target and out.extra == 5 and not PartitionOutput(None).has_target
    sub = Cluster(torch.tensor([0, 2, 3, 5]), torch.arange(5))
    out.partition = Data(y=torch.tensor([[3, 0, 0], [0, 1, 0], [0, 2, 1]]), sub=sub)
    assert out.y_superpoint.tolist() == [[3, 0, 0], [0, 1, 0], [0, 2, 1]]
    assert out.superpoint_size_histogram().tolist() == [0, 1, 2]
