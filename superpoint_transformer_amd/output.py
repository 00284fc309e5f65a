"""What stands between logits and a result in every ``validation_step`` / ``test_step`` /
``predict_step`` of the reference: ``SemanticSegmentationOutput``
(src/utils/output_semantic.py) and the multi-run inference - test-time augmentation - of
src/models/semantic.py:485-616, on the kernels of ``csrc/predict.hip`` (``predict``).

The class carries the reference's surface, names and argument names.  Differences:
  * a hop given as ``sub`` (a ``Cluster``) is walked as stored: no ``to_super_index()``;
  * an index out of range raises ``ValueError`` naming the hop (``check=True``, one host read
    at the end of the call) where the reference's gather raises ``IndexError``;
  * ``confusion_matrix`` is an addition: at voxel and raw resolution it forms the matrix against
    per-point labels without writing a prediction per point."""
import logging

import torch

from . import ops, predict

__all__ = ["SemanticSegmentationOutput", "MultiRunInference", "PanopticSegmentationOutput",
           "PartitionOutput"]

log = logging.getLogger(__name__)


class SemanticSegmentationOutput:
    """A holder for semantic segmentation model output: ``logits`` (a ``[num_nodes, C]`` tensor,
    or a list of them, level 1 first, for a multi-stage model) and ``y_hist`` (label histograms
    of the same levels, void in the last column; optional)."""

    def __init__(self, logits, y_hist=None):
        self.logits = logits
        self.y_hist = y_hist

    def debug(self):
        """Sanity checks on the attributes of self."""
        assert isinstance(self.logits, torch.Tensor) \
               or all(isinstance(l, torch.Tensor) for l in self.logits)
        if self.has_target:
            if self.multi_stage:
                assert len(self.y_hist) == len(self.logits)
                assert all(y.shape[0] == l.shape[0] for y, l in zip(self.y_hist, self.logits))
            else:
                assert self.y_hist.shape[0] == self.logits.shape[0]

    @property
    def _level1(self):
        return self.logits[0] if self.multi_stage else self.logits

    @property
    def device(self):
        return self._level1.device

    @property
    def has_target(self):
        return self.y_hist is not None

    @property
    def multi_stage(self):
        return not isinstance(self.logits, torch.Tensor)

    @property
    def num_classes(self):
        return self._level1.shape[1]

    @property
    def num_nodes(self):
        return self._level1.shape[0]

    def semantic_pred(self):
        """Semantic predictions on the level-1 superpoints: the argmax of the level-1 logits."""
        return predict.row_argmax(self._level1)

    @property
    def semantic_target(self):
        """The label histogram of the level-1 superpoints."""
        return self.y_hist[0] if self.multi_stage else self.y_hist

    @property
    def void_mask(self):
        """Mask of the level-1 nodes holding more than 50% void points (``None`` without a
        target): the last histogram column over the row total, both as f32, ``> 0.5``."""
        if not self.has_target:
            return
        return predict.void_mask(self.semantic_target)

    def __repr__(self):
        return f"{self.__class__.__name__}()"

    def voxel_semantic_pred(self, super_index=None, sub=None, check=True):
        """Level-1 predictions distributed to the level-0 points (voxels), through
        ``super_index`` (per voxel, its superpoint) or ``sub`` (the superpoints' ``Cluster``)."""
        assert super_index is not None or sub is not None, \
            "Must provide either `super_index` or `sub`"
        hop = super_index if super_index is not None else sub
        return predict.labels_through(self.semantic_pred(), [hop], want=("voxel",),
                                      check=check)["voxel"]

    @staticmethod
    def _full_res_hops(super_index_level0_to_level1=None, super_index_raw_to_level0=None,
                       sub_level1_to_level0=None, sub_level0_to_raw=None):
        assert super_index_level0_to_level1 is not None or sub_level1_to_level0 is not None, \
            "Must provide either `super_index_level0_to_level1` or `sub_level1_to_level0`"
        assert super_index_raw_to_level0 is not None or sub_level0_to_raw is not None, \
            "Must provide either `super_index_raw_to_level0` or `sub_level0_to_raw`"
        return [super_index_level0_to_level1 if super_index_level0_to_level1 is not None
                else sub_level1_to_level0,
                super_index_raw_to_level0 if super_index_raw_to_level0 is not None
                else sub_level0_to_raw]

    def full_res_semantic_pred(self, super_index_level0_to_level1=None,
                               super_index_raw_to_level0=None, sub_level1_to_level0=None,
                               sub_level0_to_raw=None, check=True):
        """Level-1 predictions distributed to the full-resolution input cloud: each of the two
        hops as a ``super_index`` tensor or as the ``sub`` Cluster of the level above."""
        hops = self._full_res_hops(super_index_level0_to_level1, super_index_raw_to_level0,
                                   sub_level1_to_level0, sub_level0_to_raw)
        return predict.labels_through(self.semantic_pred(), hops, want=("raw",),
                                      check=check)["raw"]

    def confusion_matrix(self, num_classes, target=None, resolution="segment", out=None,
                         check=True, **hops):
        """int64 ``[num_classes, num_classes]`` confusion matrix ``[true, predicted]`` of the
        level-1 predictions, accumulated into ``out`` when given.

        ``'segment'``: against label histograms (``target``, or ``y_hist`` when None) -
        ``ops.histogram_confusion_matrix``.  ``'voxel'`` / ``'raw'``: against one label per voxel
        / raw point (labels outside ``[0, num_classes)`` are void), with the hop arguments of
        ``voxel_semantic_pred`` / ``full_res_semantic_pred``; no per-point prediction is
        written."""
        pred = self.semantic_pred()
        if resolution == "segment":
            if hops:
                raise TypeError(f"resolution 'segment' takes no hops: {sorted(hops)}")
            target = self.semantic_target if target is None else target
            if target is None:
                raise ValueError("no target given and the output holds no y_hist")
            return ops.histogram_confusion_matrix(pred, target, num_classes, out=out)
        if target is None:
            raise ValueError(f"resolution {resolution!r} needs per-point target labels")
        if resolution == "voxel":
            extra = set(hops) - {"super_index", "sub"}
            if extra:
                raise TypeError(f"unexpected arguments {sorted(extra)}")
            assert hops.get("super_index") is not None or hops.get("sub") is not None, \
                "Must provide either `super_index` or `sub`"
            path = [hops["super_index"] if hops.get("super_index") is not None else hops["sub"]]
        elif resolution == "raw":
            path = self._full_res_hops(**hops)
        else:
            raise ValueError(f"resolution must be 'segment', 'voxel' or 'raw', got {resolution!r}")
        return predict.labels_through(pred, path, target=target, num_classes=num_classes,
                                      confmat=out, want=(), check=check)["confmat"]


class MultiRunInference:
    """The reference's ``step_multi_run_inference`` (src/models/semantic.py:485-561) and its
    helpers ``_create_empty_output``, ``_update_output_multi`` and
    ``_propagate_output_to_unseen_neighbors``: logits of several runs over transformed copies of
    one NAG are summed per input node, and the level-1 nodes that no run saw take the summed
    logits of their nearest seen neighbour.

    What the reference DOES where that differs from what it says: a node with no seen neighbour
    within ``r_max`` has ``neighbors == -1``, and ``logits[seen_idx][neighbors]`` then copies the
    LAST SEEN ROW - not a "label-0" prediction, as its warning puts it.  That behaviour is kept;
    the warning here states the counts and says what is copied.

    State of a multi-run output (kept on the output object): the run number and one int32 stamp
    per level, holding the last run that wrote each row.  Level 1's stamp ``!= 0`` is the
    reference's ``seen``; the other levels' stamps only tell a duplicate id from a new one."""

    def __init__(self, num_classes, multi_stage, key="tta_node_id", r_max=2):
        self.num_classes = int(num_classes)
        self.multi_stage = bool(multi_stage)
        self.key = key
        self.r_max = r_max

    def empty_output(self, nag):
        """Zero logits for every level predicted, and the run state."""
        device = nag.device
        sizes = nag.num_points[1:] if self.multi_stage else nag.num_points[1:2]
        logits = [torch.zeros(n, self.num_classes, device=device) for n in sizes]
        out = SemanticSegmentationOutput(logits if self.multi_stage else logits[0])
        out._tta_stamps = [torch.zeros(n, dtype=torch.int32, device=device) for n in sizes]
        out._tta_run = 0
        return out

    @staticmethod
    def seen(output_multi):
        """Mask of the level-1 nodes that at least one run has written."""
        return output_multi._tta_stamps[0] != 0

    def update(self, output_multi, output, nag_transformed, check=True):
        """``output_multi.logits[i][nag_transformed[i + 1][key]] += output.logits[i]`` for every
        level of ``output`` (level 1 only when it is single-stage), and the next run number."""
        output_multi._tta_run += 1
        run = output_multi._tta_run
        if output.multi_stage:
            pairs = [(output_multi.logits[i], output.logits[i], i) for i in range(len(output.logits))]
        else:
            pairs = [(output_multi._level1, output.logits, 0)]
        for acc, src, i in pairs:
            node_id = nag_transformed[i + 1][self.key]
            predict.accumulate_rows_(acc, src.detach().float(), node_id,
                                     output_multi._tta_stamps[i], run, check=check)
        return output_multi

    def _nearest_seen(self, pos, batch, seen_idx, unseen_idx):
        x_search, x_query = pos[seen_idx], pos[unseen_idx]
        b_search = batch[seen_idx] if batch is not None else None
        b_query = batch[unseen_idx] if batch is not None else None
        if pos.is_cuda:
            from .neighbors import knn_2
            return knn_2(x_search, x_query, 1, r_max=self.r_max, batch_search=b_search,
                         batch_query=b_query)[0]
        # CPU tensors: the exhaustive search, batch items kept apart as knn_2 does (a z offset)
        x_search, x_query = x_search.float().clone(), x_query.float().clone()
        if batch is not None:
            z = torch.cat((x_search[:, 2], x_query[:, 2]))
            zoff = z.max() - z.min() + self.r_max + 1
            x_search[:, 2] += b_search.to(x_search.dtype) * zoff
            x_query[:, 2] += b_query.to(x_query.dtype) * zoff
        d = (x_search.unsqueeze(0) - x_query.unsqueeze(1)).norm(dim=2)
        dmin, nn = d.min(dim=1)
        nn[dmin > self.r_max] = -1
        return nn

    def finalize(self, output_multi, nag, neighbors=None):
        """Give every unseen level-1 node the summed logits of its nearest seen neighbour
        (``knn_2(k=1, r_max)``, per batch item when ``nag[1].batch`` exists); level 1 only, like
        the reference.  A node without a seen neighbour within ``r_max`` takes the last seen row
        (class docstring).  Host reads: the unseen count and the left-out count, the
        reference's.  ``neighbors``: a precomputed ``[num_unseen]`` result of the search."""
        seen = self.seen(output_multi)
        unseen_idx = torch.where(~seen)[0]
        if unseen_idx.shape[0] == 0:
            return output_multi
        seen_idx = torch.where(seen)[0]
        if seen_idx.shape[0] == 0:
            raise ValueError("no level-1 node was seen by any run: nothing to propagate")
        if neighbors is None:
            neighbors = self._nearest_seen(nag[1].pos, nag[1].batch, seen_idx, unseen_idx)
        neighbors = neighbors.long().view(-1)
        num_left_out = int((neighbors == -1).sum())
        if num_left_out > 0:
            log.warning(
                f"Could not find a neighbor for all unseen nodes: num_seen={seen_idx.shape[0]}, "
                f"num_unseen={unseen_idx.shape[0]}, num_left_out={num_left_out}. These left out "
                f"nodes take the logits of the LAST seen node (index -1), as the reference's "
                f"indexing does. Consider sampling less nodes in the augmentations, or increase "
                f"the search radius")
        logits = output_multi._level1
        logits[unseen_idx] = logits[seen_idx][neighbors]
        return output_multi

    def run(self, model, nag, transform, num_runs):
        """``num_runs`` times: ``transform(nag.clone())``, ``model`` on the result, ``update``;
        then ``finalize``.  ``NAGSaveNodeIndex(key)`` stands in front of ``transform.transforms``
        for the duration of the loop only.  ``model`` returns a ``SemanticSegmentationOutput``,
        or logits (a tensor or the list of the levels')."""
        from .transforms import NAGSaveNodeIndex
        transform.transforms = [NAGSaveNodeIndex(key=self.key)] + list(transform.transforms)
        try:
            output_multi = self.empty_output(nag)
            for _ in range(num_runs):
                nag_ = transform(nag.clone())
                output = model(nag_)
                if not isinstance(output, SemanticSegmentationOutput):
                    if not isinstance(output, torch.Tensor) and not self.multi_stage:
                        output = output[0]
                    output = SemanticSegmentationOutput(output)
                self.update(output_multi, output, nag_)
        finally:
            transform.transforms = transform.transforms[1:]
        return self.finalize(output_multi, nag)


class PanopticSegmentationOutput(SemanticSegmentationOutput):
    """A holder for panoptic segmentation model output (src/utils/output_panoptic.py:14-508):
    the semantic output, the edge affinity logits, the node sizes, optionally the instance
    targets (``obj``: the level-1 ``InstanceData``, ``obj_edge_index``, ``obj_edge_affinity``,
    ``pos``, ``obj_pos``) and the predicted instance of each level-1 node (``obj_index_pred``),
    on the kernels of ``csrc/panoptic.hip`` (``panoptic``) and ``csrc/predict.hip``.

    Differences from the reference:
      * ``obj_index_pred`` as a list of multi-setting partition results
        (``PartitionParameterSearchStorage``) is not supported and raises;
      * ``num_edges`` is ``edge_affinity_logits.shape[0]`` (the reference reads ``shape[1]`` of
        the 1-D tensor its own ``debug`` asserts);
      * an instance's label is the first maximum of its mean logits (``predict.row_argmax``),
        where the reference takes the maximum of their softmax: the two differ only where
        rounding in the softmax creates a tie the logits do not have;
      * the per-voxel and per-point ``InstanceData`` are built directly - one pair per point,
        ``count == 1`` - and a hop given as ``sub`` is walked as stored."""

    def __init__(self, logits, stuff_classes, edge_affinity_logits, node_size, y_hist=None,
                 obj=None, obj_edge_index=None, obj_edge_affinity=None, pos=None, obj_pos=None,
                 obj_index_pred=None, semantic_loss=None, edge_affinity_loss=None):
        device = edge_affinity_logits.device
        self.stuff_classes = torch.tensor(stuff_classes, device=device).long() \
            if stuff_classes is not None else torch.empty(0, device=device).long()
        self.edge_affinity_logits = edge_affinity_logits
        self.node_size = node_size
        self.obj = obj
        self.obj_edge_index = obj_edge_index
        self.obj_edge_affinity = obj_edge_affinity
        self.pos = pos
        self.obj_pos = obj_pos
        self.obj_index_pred = obj_index_pred
        self.semantic_loss = semantic_loss
        self.edge_affinity_loss = edge_affinity_loss
        self._num_obj_pred = None
        super().__init__(logits, y_hist=y_hist)
        if self.has_multi_instance_pred:
            raise NotImplementedError(
                "obj_index_pred as a list of multi-setting partition results is not supported: "
                "pass the [num_nodes] index tensor of one setting")
        self.debug()

    def debug(self):
        super().debug()
        assert self.edge_affinity_logits.dim() == 1
        assert self.node_size.dim() == 1
        assert self.node_size.shape[0] == self.num_nodes
        if self.has_instance_pred:
            assert self.obj_index_pred.dim() == 1
            assert self.obj_index_pred.shape[0] == self.num_nodes
        items = [self.obj_edge_index, self.obj_edge_affinity, self.pos, self.obj_pos]
        if all(x is None for x in items):
            return
        assert all(x is not None for x in items)
        from .instance import InstanceData
        assert isinstance(self.obj, InstanceData)
        assert self.obj.num_clusters == self.num_nodes
        assert self.obj_edge_index.dim() == 2
        assert self.obj_edge_index.shape[0] == 2
        assert self.obj_edge_index.shape[1] == self.num_edges
        assert self.obj_edge_affinity.dim() == 1
        assert self.obj_edge_affinity.shape[0] == self.num_edges

    @property
    def has_target(self):
        """Whether ``self`` holds the targets of panoptic segmentation."""
        items = [self.obj, self.obj_edge_index, self.obj_edge_affinity, self.pos, self.obj_pos]
        return super().has_target and all(x is not None for x in items)

    @property
    def has_instance_pred(self):
        return self.obj_index_pred is not None

    @property
    def has_multi_instance_pred(self):
        return self.has_instance_pred and not isinstance(self.obj_index_pred, torch.Tensor)

    @property
    def num_edges(self):
        return self.edge_affinity_logits.shape[0]

    @property
    def edge_affinity_pred(self):
        """The sigmoid of ``edge_affinity_logits``: what the graph clustering takes."""
        return self.edge_affinity_logits.sigmoid()

    @property
    def void_edge_mask(self):
        """Mask of the edges connecting two void nodes (``None`` without a target)."""
        if not self.has_target:
            return
        mask = self.void_mask[self.obj_edge_index]
        return mask[0] & mask[1]

    def sanitized_edge_affinities(self):
        """``(edge_affinity_logits, obj_edge_affinity, is_same_class, is_same_obj)`` without the
        edges connecting two void nodes."""
        idx = torch.where(~self.void_edge_mask)[0]
        obj, count, y = self.obj.major(num_classes=self.num_classes)
        is_same_class = y[self.obj_edge_index[0]] == y[self.obj_edge_index[1]]
        is_same_obj = obj[self.obj_edge_index[0]] == obj[self.obj_edge_index[1]]
        return self.edge_affinity_logits[idx], self.obj_edge_affinity[idx], \
            is_same_class[idx], is_same_obj[idx]

    def _num_obj(self):
        if self._num_obj_pred is None:
            self._num_obj_pred = int(self.obj_index_pred.max()) + 1     # a host read, once
        return self._num_obj_pred

    def weighted_instance_semantic_pred(self, check=True):
        """``(obj_y, obj_semantic_score, obj_logits)`` of the predicted instances: the mean of
        their nodes' level-1 logits weighted by the node sizes (``panoptic.weighted_group_mean``),
        its first maximum and the maximum of its softmax (``panoptic.semantic_score``)."""
        if not self.has_instance_pred:
            return None, None, None
        from . import panoptic
        obj_logits = panoptic.weighted_group_mean(self._level1.detach().float(),
                                                  self.obj_index_pred, self.node_size,
                                                  self._num_obj(), check=check)
        obj_y = predict.row_argmax(obj_logits)
        obj_semantic_score = panoptic.semantic_score(obj_logits)
        return obj_y, obj_semantic_score, obj_logits

    def panoptic_pred(self, check=True):
        """``(obj_score, obj_y, instance_data)`` of the predicted instances; ``instance_data``
        is ``obj`` merged by ``obj_index_pred`` (``panoptic.merge_instances``), ``None`` without
        a target."""
        if not self.has_instance_pred:
            return None, None, None
        instance_data = None
        if self.has_target:
            from . import panoptic
            instance_data = panoptic.merge_instances(self.obj, self.obj_index_pred,
                                                     num_parents=self._num_obj_pred)
            self._num_obj_pred = instance_data.num_groups
        obj_y, obj_semantic_score, _ = self.weighted_instance_semantic_pred(check=check)
        return obj_semantic_score, obj_y, instance_data

    def _superpoint_labels(self, check):
        obj_y = self.weighted_instance_semantic_pred(check=check)[0]
        return predict.labels_through(obj_y, [self.obj_index_pred], want=("voxel",),
                                      check=check)["voxel"]

    @staticmethod
    def _per_point(index, y, count=None):
        from .instance import InstanceData
        n = index.shape[0]
        if count is None:
            count = torch.ones(n, dtype=torch.long, device=index.device)
        return InstanceData(torch.arange(n + 1, device=index.device), index, count, y)

    def superpoint_panoptic_pred(self, check=True):
        """``(sp_y, obj_index_pred, sp_obj_pred)``: the instances' labels on the level-1 nodes and
        the node-wise ``InstanceData`` carrying the predictions (``count`` = the node sizes)."""
        sp_y = self._superpoint_labels(check)
        return sp_y, self.obj_index_pred, self._per_point(self.obj_index_pred, sp_y,
                                                          self.node_size)

    def voxel_panoptic_pred(self, super_index=None, sub=None, check=True):
        """``(vox_y, vox_index, vox_obj_pred)``: label and instance of each level-0 point,
        through ``super_index`` or ``sub``, and the voxel-wise ``InstanceData`` (one pair per
        voxel, ``count == 1``)."""
        assert super_index is not None or sub is not None, \
            "Must provide either `super_index` or `sub`"
        hop = [super_index if super_index is not None else sub]
        vox_y = predict.labels_through(self._superpoint_labels(check), hop, want=("voxel",),
                                       check=check)["voxel"]
        vox_index = predict.labels_through(self.obj_index_pred, hop, want=("voxel",),
                                           check=check)["voxel"]
        return vox_y, vox_index, self._per_point(vox_index, vox_y)

    def full_res_panoptic_pred(self, super_index_level0_to_level1=None,
                               super_index_raw_to_level0=None, sub_level1_to_level0=None,
                               sub_level0_to_raw=None, check=True):
        """``(raw_y, raw_index, raw_obj_pred)``: the same on the full-resolution cloud, each of
        the two hops as a ``super_index`` tensor or the ``sub`` Cluster of the level above."""
        hops = self._full_res_hops(super_index_level0_to_level1, super_index_raw_to_level0,
                                   sub_level1_to_level0, sub_level0_to_raw)
        raw_y = predict.labels_through(self._superpoint_labels(check), hops, want=("raw",),
                                       check=check)["raw"]
        raw_index = predict.labels_through(self.obj_index_pred, hops, want=("raw",),
                                           check=check)["raw"]
        return raw_y, raw_index, self._per_point(raw_index, raw_y)


class PartitionOutput:
    """What the model hands to ``criterion.PartitionCriterion`` while the partition is trained
    (``PartitionOutput``, src/utils/output_partition.py): the nodes' labels ``y`` (int histograms
    ``[n, C + 1]`` or labels ``[n]``), their features ``x`` ``[n, D]`` and the graph
    ``edge_index`` ``[2, E]`` the loss contrasts them along; any further keyword becomes an
    attribute.  With a ``partition`` attribute (the level-1 ``Data`` computed from ``x`` in
    evaluation), ``y_superpoint`` and ``superpoint_size_histogram()`` read it."""

    def __init__(self, y, x=None, edge_index=None, **kwargs):
        self.y = y
        self.x = x
        self.edge_index = edge_index
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def y_superpoint(self):
        return self.partition.y

    def superpoint_size_histogram(self):
        """``bincount`` of the superpoints' sizes."""
        return torch.bincount(self.partition.sub.sizes)

    @property
    def has_target(self):
        return self.y is not None
