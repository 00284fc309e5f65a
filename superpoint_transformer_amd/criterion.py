"""The criteria of the reference's default configurations: the semantic criterion on the
histogram-loss kernels, and the panoptic one - semantic loss plus the edge-affinity loss - on
``ops.edge_affinity_loss`` (``EdgeAffinityCriterion``, ``PanopticCriterion``, below).

``configs/model/semantic/default.yaml:7-12`` trains with ``loss_type: 'ce_kl'``,
``weighted_loss: True`` and ``multi_stage_loss_lambdas: [1, 50]`` on the per-superpoint label
histograms ``nag[i].y`` (int64 [N_i, C + 1], last column void).  ``SemanticCriterion`` combines
``ops.histogram_loss`` per level exactly as ``src/models/semantic.py:397-474`` combines
``CrossEntropyLoss(weight, ignore_index=C)`` and ``loss_with_target_histogram``; on CUDA tensors
nothing in it waits on the host, so a step with it can be captured into a graph.

``'wce'`` and ``'wce_kl'`` are refused.  The reference builds their target with
``y_hist_dominant[:, y_dominant] = y.sum(dim=1)`` (``semantic.py:405-406``, ``:440-441``), an
advanced-index assignment that writes every row's total into every row and whose winner among
duplicate indices is unspecified: there is no well-defined behaviour to reproduce.
"""
import torch

from . import ops

LOSS_TYPES = ("ce", "kl", "ce_kl")
_REFUSED = ("wce", "wce_kl")


class SemanticCriterion(torch.nn.Module):
    """``criterion(logits, y_hist)``: [rows, C] logits against an int64 [rows, C or C + 1] label
    histogram (single stage: ``'ce'`` or ``'kl'``), or lists of both, one per level, finest first
    (multi stage: ``'ce'``, ``'kl'`` or ``'ce_kl'``, weighted by ``lambdas``):

    - ``'ce'``: class-weighted CE on the dominant label of each histogram, ``sum_i lambda_i CE_i``;
    - ``'kl'``: class-weighted CE against the whole histogram, ``sum_i lambda_i KL_i``;
    - ``'ce_kl'``: ``CE_0 + sum_{i >= 1} lambda_i KL_i`` (the first level carries no lambda,
      ``semantic.py:425-427``).

    ``weight``: float [C] class weights or None; a buffer, assignable after construction as the
    reference's ``on_fit_start`` does (``semantic.py:337-350``).  ``confmat``: optional int64
    [C, C] buffer (``metrics.ConfusionMatrix.confmat``) that receives, from the same pass, the
    confusion matrix of the first level's ``argmax logits`` against its histogram."""

    def __init__(self, num_classes, loss_type="ce_kl", lambdas=(1, 50), weight=None):
        super().__init__()
        if loss_type in _REFUSED:
            raise ValueError(
                f"loss_type {loss_type!r} is not supported: the reference builds its target with "
                "`y_hist_dominant[:, y_dominant] = y.sum(dim=1)`, an advanced-index assignment with "
                "duplicate indices whose result is unspecified - there is nothing well-defined to "
                "reproduce")
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"unknown loss_type {loss_type!r}: one of {LOSS_TYPES}")
        self.num_classes = int(num_classes)
        self.loss_type = loss_type
        self.lambdas = [float(l) for l in lambdas]
        self.register_buffer("weight", None)
        if weight is not None:
            self.weight = torch.as_tensor(weight, dtype=torch.float32)

    def extra_repr(self):
        return f"num_classes={self.num_classes}, loss_type={self.loss_type!r}, lambdas={self.lambdas}"

    def _level(self, kind, logits, y_hist, confmat=None):
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"logits must be [rows, {self.num_classes}], got {tuple(logits.shape)}")
        w = self.weight
        if w is not None and w.device != logits.device:
            w = w.to(logits.device)
        return ops.histogram_loss(logits, y_hist, weight=w, confmat=confmat,
                                  mode="dominant" if kind == "ce" else "histogram")

    def forward(self, logits, y_hist, confmat=None):
        multi = isinstance(logits, (list, tuple))
        if multi != isinstance(y_hist, (list, tuple)):
            raise ValueError("pass logits and histograms both as tensors or both as lists")
        if not multi:
            if self.loss_type not in ("ce", "kl"):
                raise ValueError(f"Unknown single-stage loss {self.loss_type!r}")
            return self._level(self.loss_type, logits, y_hist, confmat)
        if not len(logits) == len(y_hist) == len(self.lambdas):
            raise ValueError(f"{len(logits)} logits, {len(y_hist)} histograms, "
                             f"{len(self.lambdas)} lambdas: one of each per level")
        loss = 0
        for i, (lamb, a, b) in enumerate(zip(self.lambdas, logits, y_hist)):
            cm = confmat if i == 0 else None
            if self.loss_type == "ce_kl" and i == 0:
                loss = loss + self._level("ce", a, b, cm)
            else:
                loss = loss + lamb * self._level("ce" if self.loss_type == "ce" else "kl", a, b, cm)
        return loss


class EdgeAffinityCriterion(torch.nn.Module):
    """The edge-affinity criterion of ``PanopticSegmentationModule.model_step``
    (src/models/panoptic.py:726-796), applied to what ``sanitized_edge_affinities()`` keeps -
    without compacting: ``criterion(logits, target, obj_edge_index, node_void, node_obj, node_y)``
    or ``criterion(output)`` with a ``PanopticSegmentationOutput`` that has a target (its major
    objects then come from ``panoptic.major_objects``, its void mask from ``predict.void_mask``).

    ``weighted=False``: ``BCEWithLogitsLoss`` of src/loss/bce.py, the configs' default - the
    weights are ignored, the mean over the kept edges.  ``weighted=True``:
    ``WeightedBCEWithLogitsLoss``, ``sum(w l) / sum(w)`` with ``w`` the entry of ``case_weights``
    for ``[same-class same-obj, same-class diff-obj, diff-class same-obj, diff-class diff-obj]``
    of the end nodes' major objects; ``case_weights`` that is ``None`` or not of length 4 means no
    weighting (``_edge_affinity_weights``).  A void ``y`` takes part in the class comparison by
    its value, as in the reference.  ``pos_weight``: a number, kept as a buffer and read on the
    device.  ``stats=``: an int64 ``[4]`` buffer (``metrics.BinaryEdgeStats.state``) that takes
    tp / fp / tn / fn of the kept edges from the same pass.  Nothing waits on the host."""

    def __init__(self, weighted=False, case_weights=None, pos_weight=None):
        super().__init__()
        self.weighted = bool(weighted)
        self.register_buffer("case_weights", None)
        self.register_buffer("pos_weight", None)
        if case_weights is not None and len(case_weights) == 4:
            self.case_weights = torch.as_tensor(case_weights, dtype=torch.float32).reshape(4)
        if pos_weight is not None:
            self.pos_weight = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(1)

    def extra_repr(self):
        return f"weighted={self.weighted}"

    @staticmethod
    def targets_of(output):
        """``(node_void, node_obj, node_y)`` of a ``PanopticSegmentationOutput`` with a target."""
        from . import panoptic
        if not output.has_target:
            raise ValueError("the output holds no target: y_hist, obj, obj_edge_index, "
                             "obj_edge_affinity, pos and obj_pos are all needed")
        obj, _, y = panoptic.major_objects(output.obj, output.num_classes)
        return output.void_mask, obj, y

    def forward(self, logits, target=None, obj_edge_index=None, node_void=None, node_obj=None,
                node_y=None, stats=None):
        if not torch.is_tensor(logits):
            output = logits
            node_void, node_obj, node_y = self.targets_of(output)
            logits, target = output.edge_affinity_logits, output.obj_edge_affinity
            obj_edge_index = output.obj_edge_index
        cw = self.case_weights if self.weighted else None
        pw = self.pos_weight
        dev = logits.device
        if cw is not None and cw.device != dev:
            cw = cw.to(dev)
        if pw is not None and pw.device != dev:
            pw = pw.to(dev)
        return ops.edge_affinity_loss(logits, target, obj_edge_index, node_void, node_obj, node_y,
                                      case_weights=cw, pos_weight=pw, stats=stats)


class PanopticCriterion(torch.nn.Module):
    """``loss = semantic_loss + edge_affinity_loss_lambda * edge_affinity_loss``
    (``model_step``, src/models/panoptic.py:760-796): ``semantic`` a ``SemanticCriterion``,
    ``edge_affinity`` an ``EdgeAffinityCriterion``.  Returns ``(loss, semantic_loss,
    edge_affinity_loss)``.  ``confmat=`` goes to the semantic criterion, ``stats=`` to the
    edge-affinity criterion."""

    def __init__(self, semantic, edge_affinity, edge_affinity_loss_lambda=1):
        super().__init__()
        self.semantic = semantic
        self.edge_affinity = edge_affinity
        self.edge_affinity_loss_lambda = float(edge_affinity_loss_lambda)

    def extra_repr(self):
        return f"edge_affinity_loss_lambda={self.edge_affinity_loss_lambda}"

    def forward(self, logits, y_hist, edge_affinity_logits, obj_edge_affinity, obj_edge_index,
                node_void, node_obj, node_y, confmat=None, stats=None):
        semantic_loss = self.semantic(logits, y_hist, confmat=confmat)
        edge_affinity_loss = self.edge_affinity(edge_affinity_logits, obj_edge_affinity,
                                                obj_edge_index, node_void, node_obj, node_y,
                                                stats=stats)
        loss = semantic_loss + self.edge_affinity_loss_lambda * edge_affinity_loss
        return loss, semantic_loss, edge_affinity_loss


class BinaryFocalLoss(torch.nn.Module):
    """The reference's two-class focal loss (src/loss/focal.py:171-220), mean reduction: a holder
    of ``gamma``, ``weight`` (of the True class) and ``epsilon`` for ``PartitionCriterion``, and -
    for stand-alone use - callable on probabilities ``p`` [n] of the True label and boolean
    targets ``y`` [n] with the reference's formula."""

    def __init__(self, gamma=0, weight=0.5, epsilon=1e-6):
        super().__init__()
        self.gamma = gamma
        self.weight = weight
        self.epsilon = epsilon

    def extra_repr(self):
        return f"gamma={self.gamma}, weight={self.weight}, epsilon={self.epsilon}"

    def forward(self, p, y):
        yf = y.float()
        p = (~y).float() + p * (2 * yf - 1)
        p = self.epsilon + (1 - 2 * self.epsilon) * p
        weight = yf * self.weight + (1 - yf) * (1 - self.weight)
        return (-(1 - p) ** self.gamma * torch.log(p) * weight).mean()


class PartitionCriterion(torch.nn.Module):
    """The criterion of the partition training stage (``PartitionCriterion``,
    src/loss/partition_criterion.py): ``criterion(partition_output) -> (loss, partition_output)``
    on ``ops.partition_edge_loss`` - embeddings ``x`` that stay close along the edges inside a
    label and move apart along those across two labels.  The reference's constructor plus
    ``seed``; the adaptive sample (``adaptive_sampling_ratio``) is drawn in training mode only, on
    the device, from the module's ``state`` buffer ``(seed, calls)``.  ``sharding`` is accepted and
    ignored (nothing here gathers the edges' rows into a tensor that could be too large).

    Only ``BinaryFocalLoss`` is a ``loss_function``: its three numbers go to the kernels.

    Deviation: ``partition_output.n_inter_edge`` is a 0-dim int64 DEVICE tensor (a view of the
    module's ``counts`` buffer ``n_inter, n_intra, n_selected``, rewritten by every call), not a
    Python int - nothing waits on the host, so a step with this criterion can be captured into a
    graph.  ``status``: int32 ``[2]`` buffer, see ``ops.partition_edge_loss``."""

    INTER_EDGE_LABEL = 0
    INTRA_EDGE_LABEL = 1

    def __init__(self, loss_function=None, affinity_temperature=1, adaptive_sampling_ratio=None,
                 num_classes=None, sharding=None, seed=0):
        super().__init__()
        if loss_function is None:
            loss_function = BinaryFocalLoss()
        if not isinstance(loss_function, BinaryFocalLoss):
            raise ValueError("PartitionCriterion runs BinaryFocalLoss on the device; a "
                             f"{type(loss_function).__name__} loss function is not supported")
        if num_classes is None:
            raise ValueError("num_classes is needed: the last column of the histograms is void")
        self.loss_function = loss_function
        self.affinity_temperature = affinity_temperature
        self.adaptive_sampling_ratio = adaptive_sampling_ratio
        self.sharding = sharding
        self.num_classes = int(num_classes)
        self.register_buffer("state", torch.tensor([int(seed), 0], dtype=torch.int64))
        self.register_buffer("counts", torch.zeros(3, dtype=torch.int64))
        self.register_buffer("status", torch.zeros(2, dtype=torch.int32))

    def extra_repr(self):
        return (f"affinity_temperature={self.affinity_temperature}, "
                f"adaptive_sampling_ratio={self.adaptive_sampling_ratio}, num_classes={self.num_classes}")

    def forward(self, partition_output, selected=None):
        if not partition_output.has_target:
            raise ValueError("the partition criterion needs the labels y of the nodes")
        ratio = self.adaptive_sampling_ratio if self.training else None
        f = self.loss_function
        loss = ops.partition_edge_loss(
            partition_output.x, partition_output.y, partition_output.edge_index, self.num_classes,
            temperature=self.affinity_temperature, gamma=f.gamma, weight=f.weight, epsilon=f.epsilon,
            ratio=ratio, state=self.state if ratio is not None else None, counts=self.counts,
            status=self.status, selected=selected)
        partition_output.n_inter_edge = self.counts[0]
        return loss, partition_output
