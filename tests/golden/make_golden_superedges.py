"""Golden fixture for the horizontal graph with its stored edge features (the tail of
``RadiusHorizontalGraph``), produced by the REFERENCE'S OWN functions:
``_horizontal_graph_by_radius_for_single_level`` and ``_minimalistic_horizontal_edge_features``
(src/transforms/graph.py:872-1060, cut out by name and run unedited), ``subedges``
(src/utils/graph.py:99-463), ``Data.connect_isolated`` / ``Data.to_trimmed`` and
``cluster_radius_nn_graph``, on the import hooks and stand-ins of make_golden.py /
make_golden_adjacency.py / make_golden_subedges.py.

Scene: that of make_golden_subedges.py with one distant patch that receives no radius edge (so
``connect_isolated`` acts), and a second level: tiles grouped 2 x 2, walls in pairs, the patch
alone.  Saved per level: the graph the radius search leaves, what ``subedges`` returns, the
reference's f32 ``edge_attr``, and the same function run on float64 coordinates from the same
pairs.  ``bound`` [3] = 4 x the largest deviation of the f32 output from the f64 one, per column
group (mean_off, std_off, mean_dist): the tolerance of the feature tests, also written to
profiles/r21a_superedge_errors.txt.

Usage (build container only): python tests/golden/make_golden_superedges.py
"""
import ast
import importlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_adjacency as mga  # noqa: E402
import make_golden_subedges as mgs  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

GROUPS = ("mean_off", "std_off", "mean_dist")
COLUMNS = (slice(0, 3), slice(3, 6), slice(6, 7))
LEVELS = {1: dict(k_min=1, k_max=10, gap=0.15, ratio=0.2, se_min=20, cycles=3, margin=0.2),
          2: dict(k_min=2, k_max=8, gap=0.2, ratio=0.3, se_min=10, cycles=2, margin=0.1)}


def cut_functions(path, names, ns):
    tree = ast.parse(open(os.path.join(mg.REF, path)).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names)
    exec(compile(ast.Module(body=body, type_ignores=[]), os.path.basename(path), "exec"), ns)


class LevelData(mga.DuckData):
    num_edges = property(lambda self: 0 if self.edge_index is None else self.edge_index.shape[1])


class DuckNAG:
    """What the two functions touch of a NAG."""

    def __init__(self, data_list):
        self._list = list(data_list)

    def __getitem__(self, i):
        return self._list[i]

    absolute_num_levels = property(lambda self: len(self._list))
    has_atoms = True

    def get_super_index(self, high, low=0):
        si = self[low].super_index
        for i in range(low + 1, high):
            si = self[i].super_index[si]
        return si


def load_reference():
    nbm = mga.load_reference()
    U = sys.modules["src.utils"]
    sys.modules["torch_geometric.nn.pool.consecutive"].consecutive_cluster = O.consecutive_cluster
    for name in ("scatter", "neighbors", "edge", "sparse"):
        m = sys.modules.get(f"src.utils.{name}") or importlib.import_module(f"src.utils.{name}")
        if hasattr(m, "consecutive_cluster"):
            m.consecutive_cluster = O.consecutive_cluster
    edge = importlib.import_module("src.utils.edge")
    edge.consecutive_cluster = O.consecutive_cluster
    sys.modules["src.utils.scatter"].edge_wise_points = edge.edge_wise_points
    graph = importlib.import_module("src.utils.graph")
    U.to_trimmed = graph.to_trimmed
    keys = importlib.import_module("src.utils.keys")
    ns = {"torch": torch, "np": np, "src": sys.modules["src"], "time": time.time, "NAG": DuckNAG,
          "cluster_radius_nn_graph": nbm.cluster_radius_nn_graph,
          "sanitize_keys": keys.sanitize_keys, "SUBEDGE_FEATURES": keys.SUBEDGE_FEATURES,
          "is_trimmed": graph.is_trimmed, "base_vectors_3d": U.base_vectors_3d,
          "scatter_mean": O.scatter_mean, "scatter_std": O.scatter_std}
    cut_functions("src/transforms/graph.py", ["_horizontal_graph_by_radius_for_single_level",
                                             "_minimalistic_horizontal_edge_features"], ns)
    return graph, ns


def scene(gen):
    """make_golden_subedges' scene, a distant patch, and the second level."""
    pos, index, nseg = mgs.scene(gen)
    n = 90
    patch = torch.rand(n, 3, generator=gen) * torch.tensor([1.0, 1.0, 0.05]) \
        + torch.tensor([30.0, 30.0, 0.0])
    pos = torch.cat((pos, patch.float()))
    index = torch.cat((index, torch.full((n,), nseg)))
    perm = torch.randperm(pos.shape[0], generator=gen)
    pos, index = pos[perm], index[perm]
    grid = 5
    parent = [(i // 2) * 3 + (j // 2) for i in range(grid) for j in range(grid)]   # 9 groups
    parent += [9, 9, 10, 10, 11]                                                   # walls, patch
    return pos, index, torch.tensor(parent)


def centroids(pos, index, num):
    out = torch.zeros(num, 3, dtype=torch.float64).index_add_(0, index, pos.double())
    return (out / torch.bincount(index, minlength=num).view(-1, 1)).float()


def main():
    graph, ns = load_reference()
    gen = torch.Generator().manual_seed(777)
    pos, si0, si1 = scene(gen)
    n1, n2 = int(si0.max()) + 1, int(si1.max()) + 1
    levels = [LevelData(pos=pos, super_index=si0),
              LevelData(pos=centroids(pos, si0, n1), super_index=si1),
              LevelData(pos=centroids(pos, si1[si0], n2))]
    nag = DuckNAG(levels)
    out = dict(pos=pos, super_index_0=si0.numpy().astype(np.int32),
               super_index_1=si1.numpy().astype(np.int32), pos_1=levels[1].pos, pos_2=levels[2].pos)
    dev = np.zeros((2, 3))
    for lv, cfg in LEVELS.items():
        nag = ns["_horizontal_graph_by_radius_for_single_level"](
            nag, lv, k_min=cfg["k_min"], k_max=cfg["k_max"], gap=cfg["gap"], trim=True,
            cycles=cfg["cycles"], chunk_size=100000)
        g_ei = nag[lv].edge_index.clone()
        si = nag.get_super_index(lv)
        ei, pairs, uid = graph.subedges(pos.clone(), si.clone(), g_ei.clone(), ratio=cfg["ratio"],
                                        k_min=cfg["se_min"], cycles=cfg["cycles"],
                                        margin=cfg["margin"])
        attr = {}
        for name, p in (("f32", pos), ("f64", pos.double())):
            d = LevelData(pos=nag[lv].pos, edge_index=ei.clone())
            attr[name] = ns["_minimalistic_horizontal_edge_features"](d, p, pairs, uid).edge_attr
        assert attr["f32"].dtype == torch.float32 and attr["f64"].dtype == torch.float64
        for g, cols in enumerate(COLUMNS):
            dev[lv - 1, g] = float((attr["f32"].double() - attr["f64"])[:, cols].abs().max())
        out[f"l{lv}_graph_edge_index"] = g_ei.numpy().astype(np.int32)
        out[f"l{lv}_edge_index"] = ei.numpy().astype(np.int32)
        out[f"l{lv}_pairs"] = pairs.numpy().astype(np.int32)
        out[f"l{lv}_uid"] = uid.numpy().astype(np.int32)
        out[f"l{lv}_edge_attr"] = attr["f32"]
        out[f"l{lv}_edge_attr_f64"] = attr["f64"]
        out[f"l{lv}_cfg"] = np.asarray([cfg[k] for k in ("k_min", "k_max", "gap", "ratio", "se_min",
                                                         "cycles", "margin")], dtype=np.float64)
        sizes = torch.bincount(si)
        print(f"level {lv}: {nag[lv].num_nodes} nodes of {int(sizes.min())} .. {int(sizes.max())} "
              f"points, {ei.shape[1]} edges, {pairs.shape[1]} pairs, patch edges "
              f"{(ei == nag[lv].num_nodes - 1).any(0).sum().item()}")
    out["bound"] = 4.0 * dev.max(axis=0)
    mg.save("superedges.npz", **out)
    path = os.path.join(mg.ROOT, "profiles", "r21a_superedge_errors.txt")
    with open(path, "w") as f:
        f.write("Deviation of the reference's own f32 edge features from the same function run on\n"
                "float64 coordinates with the same pairs (tests/golden/make_golden_superedges.py,\n"
                "CPU).  max |f32 - f64| per column group; the tests' bound is 4 x the larger level.\n\n")
        f.write(f"{'level':<8}" + "".join(f"{g:>14}" for g in GROUPS) + "\n")
        for lv in LEVELS:
            f.write(f"{lv:<8}" + "".join(f"{dev[lv - 1, g]:>14.3e}" for g in range(3)) + "\n")
        f.write(f"{'bound':<8}" + "".join(f"{4 * dev[:, g].max():>14.3e}" for g in range(3)) + "\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
