"""Golden fixture for the default semantic criterion (loss_type 'ce' / 'kl' / 'ce_kl' with class
weights, configs/model/semantic/default.yaml:7-12), produced by the REFERENCE'S OWN
``loss_with_target_histogram`` (src/utils/loss.py, pure torch: loaded by file path, no ``src``
package import) and ``torch.nn.CrossEntropyLoss(weight, ignore_index)``, combined exactly as
src/models/semantic.py:397-459 writes the multi-stage branches and :460-474 the single-stage ones.

Targets are real label histograms: ``y`` of levels 1 and 2 of notebooks/demo_nag_v3.h5 (1 192 and
501 superpoints, 13 classes + void; that room has no void points and no empty superpoint), plus a
copy of level 1 in which seeded rows are emptied, made all-void or void-dominant, so that the
reference's handling of the void column is part of the record.  Logits are seeded; the reference
runs in float64 and its losses and gradients are stored in float64.

The reference's ``ConfusionMatrix`` needs torchmetrics and torch_scatter, which the build
container does not have: the fixture stores no confusion matrix, and the tests compare with the
exact integer formula ``confmat[t, p] = sum_{r: pred_r = p} h[r, t]`` instead.

Usage (build container only): python tests/golden/make_golden_criterion.py
"""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

LAMBDAS = [1, 50]                                   # multi_stage_loss_lambdas


def reference_loss_module():
    spec = importlib.util.spec_from_file_location(
        "reference_utils_loss", os.path.join(mg.REF, "src/utils/loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def multi_stage(loss_type, hist_loss, criteria, logits, y_hist):
    """The multi-stage branches of src/models/semantic.py:397-459, as written there."""
    if loss_type == "ce":
        loss = 0                                    # MultiLoss.forward (src/loss/multi.py:33-37)
        for lamb, criterion, a, b in zip(LAMBDAS, criteria, logits, [y.argmax(dim=1) for y in y_hist]):
            loss = loss + lamb * criterion(a, b)
        return loss
    loss = 0
    for i, (lamb, criterion, a, b) in enumerate(zip(LAMBDAS, criteria, logits, y_hist)):
        if loss_type == "ce_kl" and i == 0:
            loss = loss + criterion(a, b.argmax(dim=1))
            continue
        loss = loss + lamb * hist_loss(criterion, a, b)
    return loss


def main():
    sys.path.insert(0, mg.ROOT)
    from superpoint_transformer_amd import h5io
    ref = reference_loss_module()
    nag = h5io.load_nag(os.path.join(mg.REF, "notebooks", "demo_nag_v3.h5"))
    y1, y2 = nag[1].y.long(), nag[2].y.long()
    C = y1.shape[1] - 1
    gen = torch.Generator().manual_seed(47)
    y1v = y1.clone()
    pick = torch.randperm(y1.shape[0], generator=gen)[:90]
    y1v[pick[:30]] = 0                                           # empty rows
    y1v[pick[30:60], C] = y1v[pick[30:60]].sum(dim=1)            # all-void rows
    y1v[pick[30:60], :C] = 0
    y1v[pick[60:], C] = y1v[pick[60:]].max(dim=1).values + 1     # void-dominant rows
    z1 = torch.randn(y1.shape[0], C, generator=gen) * 3
    z2 = torch.randn(y2.shape[0], C, generator=gen) * 3
    weight = 0.4 + 1.6 * torch.rand(C, generator=gen)
    out = dict(y1=y1.int(), y2=y2.int(), y1v=y1v.int(), z1=z1, z2=z2, weight=weight,
               lambdas=torch.tensor(LAMBDAS))

    for wname, w in (("w", weight.double()), ("u", None)):
        criteria = [torch.nn.CrossEntropyLoss(weight=w, ignore_index=C) for _ in LAMBDAS]
        # single stage (semantic.py:460-474) per case
        for cname, z, y in (("l1", z1, y1), ("l2", z2, y2), ("l1v", z1, y1v)):
            zd = z.double()
            out[f"{wname}_single_ce_{cname}"] = criteria[0](zd, y.argmax(dim=1))
            out[f"{wname}_single_kl_{cname}"] = ref.loss_with_target_histogram(criteria[0], zd, y)
        # multi stage on (level 1 with void rows, level 2)
        for loss_type in ("ce", "kl", "ce_kl"):
            a = [z1.double().requires_grad_(), z2.double().requires_grad_()]
            loss = multi_stage(loss_type, ref.loss_with_target_histogram, criteria, a, [y1v, y2])
            out[f"{wname}_multi_{loss_type}"] = loss.detach()
            if wname == "w":
                g1, g2 = torch.autograd.grad(loss, a)
                out[f"w_multi_{loss_type}_g1"], out[f"w_multi_{loss_type}_g2"] = g1, g2
    mg.save("criterion.npz", **out)


if __name__ == "__main__":
    main()
