"""Deviations behind the float bars of the panoptic tests (tests/panoptic_cases.py): for every
float quantity of tests/golden/panoptic.npz, the largest deviation of the reference's own f32
result and of this package's result from the fixture's float64 evaluation.

    python tools/panoptic_errors.py [--cpu] > profiles/r19a_panoptic_errors.txt
"""
import contextlib
import io
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import panoptic_cases as pc  # noqa: E402


def main():
    dev = "cpu" if "--cpu" in sys.argv else torch.device("cuda:0")
    rows = []
    with contextlib.redirect_stdout(io.StringIO()):
        for variant in sorted(pc.VARIANTS):
            _, report = pc.check_metric(dev, variant)
            rows += [(f"{variant} {k}", *v) for k, v in report.items()]
        rows += [(k, *v) for k, v in pc.check_big_mean(dev).items()]
        o = pc.output(dev)
        score = o.weighted_instance_semantic_pred()[1]
        rows.append(("obj_score (fixture instances)",
                     *pc.within(score, pc.golden()["obj_score"], pc.golden()["f64__obj_score"], "")))
    where = "CPU route" if dev == "cpu" else torch.cuda.get_device_name(0)
    print(f"largest |value - float64 yardstick| per quantity; package on: {where}")
    print("bar of the tests, per element: max(4 x reference deviation, one f32 ulp of the value)")
    print(f"{'quantity':<46}{'reference (f32)':>18}{'package':>14}")
    for name, got, ref in rows:
        # (the reference's two sums are not among its results: SQ and PQ-modified carry them)
        ref = f"{'-':>18}" if name.endswith("_sum") else f"{ref:>18.3e}"
        print(f"{name:<46}{ref}{got:>14.3e}")


if __name__ == "__main__":
    main()
