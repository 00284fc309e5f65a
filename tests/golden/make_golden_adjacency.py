"""Golden fixture for the partition's input graph, produced by the REFERENCE'S OWN
``knn_1`` / ``knn_2`` / ``isolated_nodes`` / ``to_trimmed`` (src/utils/neighbors.py, graph.py,
imported verbatim by path) and ``AdjacencyGraph._process`` (src/transforms/graph.py:67-96),
``Data.is_isolated`` / ``connect_isolated`` / ``to_trimmed`` (src/data/data.py:472-586).

The two classes' modules cannot be imported here (they subclass torch_geometric's Data and pull
h5py / hydra at import time), so the methods' FunctionDefs are cut out of the files with ``ast``
- unmodified - and executed as methods of a duck-typed attribute store, like
make_golden_select.py does for ``Data.select``.

Stand-ins (all "[third-party restated]" in oracle/spt_oracle.py): torch_geometric's coalesce /
remove_self_loops and the FRNN CUDA search (exhaustive float32 search with FRNN's contract).
``Tensor.cuda`` is made a no-op for the calls because knn_1 / knn_2 move CPU inputs to the GPU.
``torch.linalg.lstsq`` is wrapped to record the (a, b) the reference fits.

Clouds: ~2 k points in a slab, a handful of far outliers that find nobody within the search
radius, and one far PAIR whose members are each other's nearest node: both are isolated, both
new edges are the same pair - the duplicate among new edges.  Indices are stored as int32.

Usage (build container only): python tests/golden/make_golden_adjacency.py
"""
import ast
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from oracle import spt_oracle as O  # noqa: E402

REF = mg.REF
REDUCE = ["mean", "add", "min", "max"]


def cut(path, cls, name):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    c = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    fn = next(n for n in c.body if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    return ast.Module(body=[fn], type_ignores=[])


def frnn_stand_in(points1, points2, K=None, r=None, **kw):
    d, i = O.frnn_grid_points(points1[0], points2[0], int(K.view(-1)[0]), float(r.view(-1)[0]))
    return d.unsqueeze(0), i.unsqueeze(0), None, None


class DuckData:
    """Attribute store with the properties the three methods touch (data.py:143-175)."""

    def __init__(self, **kw):
        self.__dict__.update(edge_index=None, edge_attr=None, batch=None, neighbor_distance=None)
        self.__dict__.update(kw)

    num_nodes = property(lambda self: self.pos.shape[0])
    device = property(lambda self: self.pos.device)
    has_neighbors = property(lambda self: self.neighbor_index is not None
                             and self.neighbor_index.shape[1] > 0)
    has_edges = property(lambda self: self.edge_index is not None and self.edge_index.shape[1] > 0)
    edge_keys = property(lambda self: [])

    def raise_if_edge_keys(self):
        pass


def load_reference():
    U, _ = mg.install_reference_import_hooks()
    tgu = sys.modules["torch_geometric.utils"]
    tgu.coalesce = O.coalesce
    tgu.remove_self_loops = O.remove_self_loops
    sys.modules["torch_geometric.nn.pool.consecutive"].consecutive_cluster = O.consecutive_cluster
    for name in ("scatter", "neighbors", "edge"):
        m = sys.modules.get(f"src.utils.{name}") or importlib.import_module(f"src.utils.{name}")
        if hasattr(m, "coalesce"):
            m.coalesce = O.coalesce
    edge = importlib.import_module("src.utils.edge")
    U.edge_wise_points = edge.edge_wise_points
    graph = importlib.import_module("src.utils.graph")
    nbm = sys.modules["src.utils.neighbors"]
    nbm.frnn.frnn_grid_points = frnn_stand_in
    torch.Tensor.cuda = lambda self, *a, **k: self

    ns = {"torch": torch, "src": sys.modules["src"], "knn_2": nbm.knn_2,
          "isolated_nodes": graph.isolated_nodes, "to_trimmed": graph.to_trimmed}
    exec(compile(cut("src/transforms/graph.py", "AdjacencyGraph", "_process"), "graph.py", "exec"), ns)
    DuckData.adjacency = ns["_process"]
    for name in ("is_isolated", "connect_isolated", "to_trimmed"):
        ns2 = dict(ns)
        exec(compile(cut("src/data/data.py", "Data", name), "data.py", "exec"), ns2)
        setattr(DuckData, name, ns2[name])
        ns2[name] = ns.get(name)        # the method's own name must keep meaning the utility
    return nbm


def cloud(gen, n, n_out, origin=0.0):
    """A slab of n points (about 11 per ball of r = 0.6: full and partial neighbourhoods), far
    outliers, a far pair."""
    pos = torch.rand(n, 3, generator=gen) * torch.tensor([9.0, 9.0, 2.0])
    out = torch.rand(n_out, 3, generator=gen) * 40.0 + torch.tensor([30.0, 30.0, 30.0])
    pair = torch.tensor([[80.0, 5.0, 5.0], [80.0, 5.0, 7.5]])
    p = torch.cat((pos, out, pair)) + origin
    return p[torch.randperm(p.shape[0], generator=gen)].float()


def main():
    nbm = load_reference()
    gen = torch.Generator().manual_seed(20240611)
    cases = [dict(n=2000, K=12, k=10, w=1.0, reduce="mean", k_iso=1, r=0.6),
             dict(n=2000, K=4, k=4, w=-1.0, reduce="add", k_iso=1, r=0.5),
             dict(n=2000, K=10, k=10, w=1.0, reduce="max", k_iso=2, r=0.6),
             dict(n=2400, K=10, k=10, w=1.0, reduce="mean", k_iso=1, r=0.6, batch=True)]
    out = {}
    orig_lstsq = torch.linalg.lstsq
    for c, cfg in enumerate(cases):
        if cfg.get("batch"):
            half = cfg["n"] // 2
            pos = torch.cat((cloud(gen, half, 4), cloud(gen, half, 5)))
            batch = torch.cat((torch.zeros(half + 6, dtype=torch.long),
                               torch.ones(half + 7, dtype=torch.long)))
        else:
            pos, batch = cloud(gen, cfg["n"], 6), None
        nn, dist = nbm.knn_1(pos, cfg["K"], r_max=cfg["r"], batch=batch)
        data = DuckData(pos=pos, batch=batch, neighbor_index=nn.clone(),
                        neighbor_distance=dist.clone())
        data.k, data.w = cfg["k"], cfg["w"]                      # AdjacencyGraph's own fields
        data = DuckData.adjacency(data, data)
        iso = data.is_isolated()
        fitted = []

        def recording(a, b):
            res = orig_lstsq(a, b)
            fitted.append(res.solution.clone())
            return res
        torch.linalg.lstsq = recording
        try:
            data = data.connect_isolated(k=cfg["k_iso"])
        finally:
            torch.linalg.lstsq = orig_lstsq
        data = data.to_trimmed(reduce=cfg["reduce"])
        assert int(iso.sum()) >= 6 and len(fitted) == 1
        out[f"c{c}_pos"] = pos
        out[f"c{c}_nn"] = nn.numpy().astype(np.int32)
        out[f"c{c}_dist"] = dist
        if batch is not None:
            out[f"c{c}_batch"] = batch.numpy().astype(np.int32)
        out[f"c{c}_edge_index"] = data.edge_index.numpy().astype(np.int32)
        out[f"c{c}_edge_attr"] = data.edge_attr
        out[f"c{c}_is_isolated"] = iso
        out[f"c{c}_ab"] = fitted[0]
        out[f"c{c}_cfg"] = np.asarray([cfg["k"], cfg["w"], cfg["k_iso"], REDUCE.index(cfg["reduce"])],
                                      dtype=np.float64)
        print(f"case {c}: {pos.shape[0]} points, {int(iso.sum())} isolated, "
              f"{data.edge_index.shape[1]} edges, (a, b) = {fitted[0].tolist()}")
    mg.save("adjacency.npz", **out)


if __name__ == "__main__":
    main()
