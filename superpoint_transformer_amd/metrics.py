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
