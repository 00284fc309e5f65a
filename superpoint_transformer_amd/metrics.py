"""Semantic segmentation metrics from segment-level predictions and label histograms.

``ConfusionMatrix`` mirrors the reference's ``src/metrics/semantic.py`` (``update`` on
histograms or 1-D labels, ``iou`` / ``oa`` / ``miou`` / ``macc`` / ``all_metrics`` with its
formulas) without torchmetrics: the state is one int64 [C, C] tensor (``[true, predicted]``)
that lives on the device and is accumulated by ``ops.histogram_confusion_matrix`` in exact
integers (the reference sums in float32 before ``.long()``).  Labels in [0, num_classes) are
valid; anything else, and histogram columns past ``num_classes``, is void.
"""
from types import SimpleNamespace

import torch

from . import ops


class ConfusionMatrix:
    def __init__(self, num_classes, device=None):
        self.num_classes = int(num_classes)
        self.confmat = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64,
                                   device=device)

    def to(self, device):
        self.confmat = self.confmat.to(device)
        return self

    def reset(self):
        self.confmat.zero_()

    def update(self, pred, target):
        """``pred``: int labels [rows] or [rows, num_classes] logits; ``target``: int64 label
        histograms [rows, >= num_classes] or labels [rows] / [rows, 1].  The state follows the
        inputs' device."""
        if self.confmat.device != pred.device:
            self.confmat = self.confmat.to(pred.device)
        ops.histogram_confusion_matrix(pred, target, self.num_classes, out=self.confmat)

    __call__ = update

    def compute(self):
        return self.confmat

    @classmethod
    def from_confusion_matrix(cls, confusion_matrix):
        assert confusion_matrix.dim() == 2 and confusion_matrix.shape[0] == confusion_matrix.shape[1]
        assert not confusion_matrix.is_floating_point()
        cm = cls(confusion_matrix.shape[0], device=confusion_matrix.device)
        cm.confmat = confusion_matrix.long().contiguous().clone()
        return cm

    @classmethod
    def from_histogram(cls, h):
        """Every histogram predicted as its dominant label (all ``h.shape[1]`` columns are classes)."""
        assert h.dim() == 2 and not h.is_floating_point()
        cm = cls(h.shape[1], device=h.device)
        cm.update(h.argmax(dim=1), h)
        return cm

    def iou(self, as_percent=True):
        """(per-class IoU, mask of the classes that exist in prediction or ground truth)."""
        tp_fn = self.confmat.sum(dim=0)
        tp_fp = self.confmat.sum(dim=1)
        tp = self.confmat.diag()
        union = tp_fn + tp_fp - tp
        iou = 1e-8 + tp / (union + 1e-8)
        if as_percent:
            iou = iou * 100
        return iou, union > 1e-3

    def oa(self, as_percent=True):
        total = int(self.confmat.sum())
        diag = int(self.confmat.diag().sum())
        return float(diag * (100 if as_percent else 1)) / (total if total else 1)

    def miou(self, missing_as_one=False, as_percent=True):
        """Mean IoU over the classes that exist; ``missing_as_one`` counts an absent class as 1
        (the literal 1 of the reference, also in percent) over all classes.  0 if none exists."""
        values, exists = self.iou(as_percent=as_percent)
        if int(exists.sum()) == 0:
            return 0
        if missing_as_one:
            return torch.where(exists, values, torch.ones_like(values)).sum() / exists.numel()
        return torch.where(exists, values, torch.zeros_like(values)).sum() / exists.sum()

    def macc(self, as_percent=True):
        """Mean per-class accuracy over the classes present in the ground truth (0 if none)."""
        total_gt = self.confmat.sum(dim=1)
        present = total_gt > 0
        if int(present.sum()) == 0:
            return 0
        acc = self.confmat.diag() / total_gt.clamp(min=1)
        re = torch.where(present, acc, torch.zeros_like(acc)).sum()
        if as_percent:
            re = re * 100
        return re / present.sum()

    def all_metrics(self, as_percent=True):
        iou, seen = self.iou(as_percent=as_percent)
        return SimpleNamespace(oa=self.oa(as_percent=as_percent), macc=self.macc(as_percent=as_percent),
                               miou=self.miou(as_percent=as_percent), iou_per_class=iou,
                               seen_class=seen)


class PanopticMetricResults:
    """The fields of the reference's ``PanopticMetricResults`` (src/metrics/panoptic.py:18-42)."""
    __slots__ = ("pq", "sq", "rq", "pq_modified", "pq_thing", "sq_thing", "rq_thing", "pq_stuff",
                 "sq_stuff", "rq_stuff", "pq_per_class", "sq_per_class", "rq_per_class",
                 "precision_per_class", "recall_per_class", "tp_per_class", "fp_per_class",
                 "fn_per_class", "pq_modified_per_class", "mean_precision", "mean_recall")


class PanopticQuality3D:
    """The reference's ``PanopticQuality3D`` (src/metrics/panoptic.py:45-381) without
    torchmetrics and without a list of scenes: Panoptic Quality is additive over scenes - objects
    of different scenes never meet - so the state is five ``[num_classes]`` counters on the
    device (``panoptic.new_state``), and ``update`` adds a batch into them by
    ``panoptic.pair_stats`` and ``panoptic.panoptic_counts_`` with no host read.

    ``y`` in ``[0, num_classes)`` are valid labels, anything else is void.  ``compute`` reads the
    state (and the fault counts of the updates) ONCE and forms every field of
    ``PanopticMetricResults`` on the host, in float64, with the reference's handling of
    ``0 / 0``, of unseen classes (``ignore_unseen_classes``) and of ``stuff_classes``.

    ``tp``, ``gt_count``, ``pred_count``, ``iou_sum``, ``iou_mod_sum`` are views of the state:
    with several ranks, sum them (one all-reduce of ``state`` viewed as its two dtypes)."""

    def __init__(self, num_classes, ignore_unseen_classes=True, stuff_classes=None, device=None):
        from . import panoptic
        self.num_classes = int(num_classes)
        self.ignore_unseen_classes = ignore_unseen_classes
        self.stuff_classes = [int(c) for c in (stuff_classes if stuff_classes is not None else [])]
        self._stuff = torch.tensor([c in self.stuff_classes for c in range(self.num_classes)],
                                   dtype=torch.bool)
        self.state = panoptic.new_state(self.num_classes, device)
        self.status = torch.zeros(panoptic.STATUS_WORDS, dtype=torch.int32, device=device)
        self._stuff_dev = self._stuff.to(self.state.device)

    def to(self, device):
        self.state = self.state.to(device)
        self.status = self.status.to(device)
        self._stuff_dev = self._stuff.to(device)
        return self

    @property
    def device(self):
        return self.state.device

    def _views(self):
        from . import panoptic
        return panoptic.state_views(self.state)

    tp = property(lambda self: self._views()[0])
    gt_count = property(lambda self: self._views()[1])
    pred_count = property(lambda self: self._views()[2])
    iou_sum = property(lambda self: self._views()[3])
    iou_mod_sum = property(lambda self: self._views()[4])

    def reset(self):
        self.state.zero_()
        self.status.zero_()

    def update(self, prediction_semantic, instance_data):
        """``prediction_semantic``: int64 ``[num_clusters]`` labels of the predicted instances;
        ``instance_data``: their overlaps with ALL target objects of the scene(s), 'stuff'
        included - predictions and targets are two partitions of the points.  The state follows
        the inputs' device before the first update."""
        from . import panoptic
        from .instance import InstanceData
        if not isinstance(prediction_semantic, torch.Tensor):
            raise ValueError("Expected argument `prediction_semantic` to be of type Tensor")
        if not isinstance(instance_data, InstanceData):
            raise ValueError("Expected argument `instance_data` to be of type InstanceData")
        if self.state.device != instance_data.device:
            self.to(instance_data.device)
        stats = panoptic.pair_stats(instance_data, self.num_classes, status=self.status)
        panoptic.panoptic_counts_(self.state, prediction_semantic, instance_data,
                                  self.num_classes, self._stuff_dev, stats=stats)

    __call__ = update

    def compute(self):
        from . import panoptic
        c = self.num_classes
        words = torch.cat((self.state.view(-1), self.status.long())).tolist()   # THE host read
        panoptic.raise_status("PanopticQuality3D", words[5 * c:])
        ints = torch.tensor(words[:3 * c], dtype=torch.int64).view(3, c)
        sums = torch.tensor(words[3 * c:5 * c], dtype=torch.int64).view(torch.float64).view(2, c)
        tp, gt_class_counts, pred_class_counts = ints[0], ints[1], ints[2]
        iou_sum, iou_mod_sum = sums[0], sums[1]
        is_stuff = self._stuff
        has_stuff = bool(is_stuff.any())

        precision = tp.double() / pred_class_counts.double()
        precision[precision.isnan()] = 0
        recall = tp.double() / gt_class_counts.double()
        fp = pred_class_counts - tp
        fn = gt_class_counts - tp
        sq = iou_sum / tp.double()
        sq[sq.isnan()] = 0
        rq = 2 * precision * recall / (precision + recall)
        rq[rq.isnan()] = 0
        pq = sq * rq
        if has_stuff:
            denominator = (gt_class_counts + pred_class_counts).double() / 2
            denominator[is_stuff] = gt_class_counts[is_stuff].double()
            pq_mod = iou_mod_sum / denominator
        else:
            pq_mod = pq.clone()

        is_seen = (gt_class_counts + pred_class_counts) > 0
        default = float("nan") if self.ignore_unseen_classes else 0
        for t in (pq, sq, rq, pq_mod, precision, recall):
            t[~is_seen] = default
        if not self.ignore_unseen_classes:
            for t in (pq, sq, rq, pq_mod, precision):
                assert not t.isnan().any()

        nan = torch.tensor(float("nan"), dtype=torch.float64)
        m = PanopticMetricResults()
        m.pq, m.sq, m.rq, m.pq_modified = pq.nanmean(), sq.nanmean(), rq.nanmean(), pq_mod.nanmean()
        m.pq_thing, m.sq_thing, m.rq_thing = (t[~is_stuff].nanmean() for t in (pq, sq, rq))
        m.pq_stuff, m.sq_stuff, m.rq_stuff = ((t[is_stuff].nanmean() if has_stuff else nan)
                                              for t in (pq, sq, rq))
        m.pq_per_class, m.sq_per_class, m.rq_per_class = pq, sq, rq
        m.precision_per_class, m.recall_per_class = precision, recall
        m.tp_per_class, m.fp_per_class, m.fn_per_class = tp, fp, fn
        m.pq_modified_per_class = pq_mod
        m.mean_precision, m.mean_recall = precision.nanmean(), recall.nanmean()
        return m


class BinaryEdgeStats:
    """The edge-affinity metrics the panoptic module logs every step (``BinaryAccuracy`` and
    ``BinaryF1Score`` on the sanitized edge affinities, src/models/panoptic.py:844-850) from four
    int64 counters on the device: ``state = [tp, fp, tn, fn]`` of ``logit > 0`` against
    ``target > 0.5`` over the edges that do not join two void nodes.  ``ops.edge_affinity_loss``
    (``stats=metric.state``) fills them from the pass that computes the loss; ``update`` does the
    same without a loss.  Neither reads the device from the host; ``compute`` reads it once.

    One corner differs from torchmetrics: it applies a sigmoid to its input only when some value
    lies outside [0, 1], so a batch whose logits ALL lie in [0, 1] is thresholded at 0.5 there.
    Here the logit is always thresholded at 0.

    ``oa()`` and ``f1()`` are float64; 0 / 0 (no edge counted; no positive in prediction or
    target) gives 0.0, as torchmetrics' safe division does."""

    def __init__(self, device=None):
        self.state = torch.zeros(4, dtype=torch.int64, device=device)

    def to(self, device):
        self.state = self.state.to(device)
        return self

    def reset(self):
        self.state.zero_()

    def update(self, logits, target, edge_index, node_void):
        """Add the kept edges of one batch (no host read)."""
        if self.state.device != logits.device:
            self.to(logits.device)
        n = node_void.shape[0]
        zeros = torch.zeros(n, dtype=torch.int64, device=logits.device)
        ops.edge_affinity_loss(logits.detach(), target, edge_index, node_void, zeros, zeros,
                               stats=self.state)

    __call__ = update

    def compute(self):
        """``(tp, fp, tn, fn)`` as Python integers: THE host read."""
        return tuple(self.state.tolist())

    def oa(self):
        tp, fp, tn, fn = self.compute()
        total = tp + fp + tn + fn
        return float(tp + tn) / total if total else 0.0

    def f1(self):
        tp, fp, tn, fn = self.compute()
        den = 2 * tp + fp + fn
        return float(2 * tp) / den if den else 0.0
