"""configs_resolved.json: the reference's Hydra trees composed and resolved by tests/hydra_lite.py
for the compositions tests/test_configs_reference.py checks: the values it reads, resolved.  Needs the reference's configs/ (hydra_lite.ROOT)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hydra_lite as H  # noqa: E402

KITTI = {"model": {"_down_dim": [128] * 4, "_up_dim": [128] * 3,
                   "net": {"no_ffn": False, "down_ffn_ratio": 1}}}
COMPOSITIONS = [("semantic/s3dis", "semantic/spt-2", None),
                ("semantic/kitti360", "semantic/spt-2", KITTI),
                ("semantic/s3dis_nano", "semantic/nano-2", None),
                ("panoptic/s3dis", "panoptic/spt-2", None),
                ("semantic/dales", "semantic/spt-2", None)]

# what the tests read (nothing else of the trees is recorded)
KEYS = ["datamodule." + k for k in ("num_hf_point", "num_hf_edge", "num_hf_segment", "num_classes", "voxel",
                                    "knn", "knn_r", "knn_step", "instance_k_max", "instance_radius")] + \
       ["model." + k for k in ("net", "multi_stage_loss_lambdas", "edge_affinity_head",
                               "edge_affinity_loss_lambda")]


def resolved(c, path, node):
    """Every leaf under ``path`` resolved; a leaf that does not resolve (runtime-only
    interpolations) is left out."""
    if isinstance(node, dict):
        out = {}
        for k, v in node.items():
            r = resolved(c, f"{path}.{k}", v)
            if r is not _MISSING:
                out[k] = r
        return out
    try:
        return c.get(path)
    except Exception:
        return _MISSING


_MISSING = object()

if __name__ == "__main__":
    out = {}
    for dm, model, over in COMPOSITIONS:
        c = H.compose(dm, model, over)
        rec = {"datamodule": {}, "model": {}}
        for key in KEYS:
            node, leaf = key.split(".")
            try:
                raw = c.raw(key)
            except (KeyError, IndexError):
                continue                            # not in this composition
            r = resolved(c, key, raw)
            if r is not _MISSING:
                rec[node][leaf] = r
        out[H.recorded_key(dm, model, over)] = rec
    with open(os.path.join(HERE, "configs_resolved.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
