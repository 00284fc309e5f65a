"""The pool-fused top layer's FORWARD entry (`spt_fused_linear_fwd_pool_runs_f32`: kernels
`fpool::fwd_pool_kernel`, the Gram / statistics finish, `pool_apply_kernel` of csrc/fused_pool.hip)
at level size - 3 M rows, ~35 rows per segment, K = 64 -> N = 128 (and once 32 -> 64) - where every
wave walks hundreds of tiles, carries an open segment across them, prefetches a tile ahead and cuts
its range at segment boundaries; in the f32 mode, the bf16 mode and with bf16 activation storage,
rows shuffled and in CSR order, one run and three runs (tests/fpool_harness.py describes the
problem: empty segments everywhere, a 120 000-row segment, bitwise equal rows, negative and zero
norm weights, run boundaries off the 16-row grid, a run of a few thousand rows).

Reference: tests/fpool_reference.py (f64, pinned on the oracle by tests/test_fpool_reference_cpu.py),
evaluated on the GPU from the call's own inputs.  Checked per call: `raw` = h64 of the reported
position; the position is a WITNESS of the extremum (inside its segment; sgn h64 there is within
2 E of the segment's extremum, E the bound of raw: the kernel prefers row a to the true winner b only
if its own h(a) >= h(b), each within E of h64); exactly the first position on zero-weight channels
and among bitwise equal rows; arg = perm[argpos]; out = y(raw) to one f32 ulp; sentinels of empty
segments; Gram record, totals and the four norm tables per graph; NULL `arg` and a repeated call
are bitwise the same.

Error = max |got - ref| / max |ref| (raw, out: / max |h64|; per graph, the worst graph).  The bound
is twice the error of the library of the commit BEFORE this file (cbc4cef, measured with this very
test on one MI355X; profiles/r08a_fpool_fwd_level_errors.txt): a change of summation order moves an
f32 sum's error by about its own size, a wrong operand plane or a dropped row by orders of
magnitude.  Sanity of the recorded values: f32-mode raw < 1e-5, bf16-mode raw < 2e-2.
(The bf16 mode's raw / out maxima are single roundings: the bulk of the winners is as close as in the
f32 mode - median 4.9e-9 - and a few hundred rows have one y that the kernel's f32 fma and the f64
reference round to different bf16 neighbours; with bf16 storage no winner met one.)

    case                        raw       out       G         sum_y     sum_h     sum_h2    mean      rstd      am        scale    
    f32-shuffled-1run-64x128    3.082e-07 7.955e-07 1.074e-06 5.197e-08 2.017e-08 4.062e-07 3.262e-08 6.820e-07 3.951e-08 6.568e-07
    f32-shuffled-3run-64x128    2.342e-07 1.234e-06 2.736e-06 5.925e-08 2.919e-08 7.163e-07 5.147e-08 1.217e-06 6.207e-08 1.227e-06
    f32-csr-1run-64x128         2.951e-07 7.022e-07 1.135e-06 4.114e-08 3.013e-08 5.759e-07 4.830e-08 7.002e-07 7.749e-08 6.626e-07
    f32-csr-3run-64x128         2.511e-07 1.184e-06 2.404e-06 9.738e-08 4.356e-08 9.105e-07 5.065e-08 1.300e-06 6.975e-08 1.142e-06
    bf16-shuffled-1run-64x128   9.047e-04 7.884e-04 1.877e-07 5.110e-08 3.012e-08 3.977e-08 5.494e-08 8.096e-08 4.283e-08 6.948e-08
    bf16-shuffled-3run-64x128   7.220e-04 1.308e-03 2.506e-07 7.478e-08 4.639e-08 8.172e-08 5.403e-08 1.690e-07 4.667e-08 1.420e-07
    bf16-csr-1run-64x128        1.045e-03 4.631e-04 1.160e-07 3.372e-08 2.337e-08 5.967e-08 5.725e-08 8.626e-08 7.652e-08 8.539e-08
    bf16-csr-3run-64x128        1.080e-03 8.382e-04 1.859e-07 6.342e-08 5.079e-08 1.055e-07 6.030e-08 1.488e-07 6.052e-08 8.684e-08
    bf16x-shuffled-3run-64x128  1.073e-07 2.007e-07 2.963e-07 6.486e-08 2.913e-08 1.090e-07 3.426e-08 1.715e-07 5.443e-08 1.044e-07
    f32-shuffled-3run-32x64     1.049e-07 1.264e-06 1.721e-06 9.095e-08 4.191e-08 9.484e-07 5.354e-08 1.103e-06 4.743e-08 1.196e-06
"""
import pytest
import torch

import fpool_harness as H
from superpoint_transformer_amd import _lib

ROWS, SEGS, GIANT = 3_000_000, 3_000_000 // 35, 120_000

# the parent commit's errors, in the order of fpool_harness.QUANTITIES:
#   raw out G sum_y sum_h sum_h2 mean rstd am scale
PARENT_ERR = {
    "f32-shuffled-1run-64x128": (3.082e-07, 7.955e-07, 1.074e-06, 5.197e-08, 2.017e-08, 4.062e-07, 3.262e-08, 6.820e-07, 3.951e-08, 6.568e-07),
    "f32-shuffled-3run-64x128": (2.342e-07, 1.234e-06, 2.736e-06, 5.925e-08, 2.919e-08, 7.163e-07, 5.147e-08, 1.217e-06, 6.207e-08, 1.227e-06),
    "f32-csr-1run-64x128": (2.951e-07, 7.022e-07, 1.135e-06, 4.114e-08, 3.013e-08, 5.759e-07, 4.830e-08, 7.002e-07, 7.749e-08, 6.626e-07),
    "f32-csr-3run-64x128": (2.511e-07, 1.184e-06, 2.404e-06, 9.738e-08, 4.356e-08, 9.105e-07, 5.065e-08, 1.300e-06, 6.975e-08, 1.142e-06),
    "bf16-shuffled-1run-64x128": (9.047e-04, 7.884e-04, 1.877e-07, 5.110e-08, 3.012e-08, 3.977e-08, 5.494e-08, 8.096e-08, 4.283e-08, 6.948e-08),
    "bf16-shuffled-3run-64x128": (7.220e-04, 1.308e-03, 2.506e-07, 7.478e-08, 4.639e-08, 8.172e-08, 5.403e-08, 1.690e-07, 4.667e-08, 1.420e-07),
    "bf16-csr-1run-64x128": (1.045e-03, 4.631e-04, 1.160e-07, 3.372e-08, 2.337e-08, 5.967e-08, 5.725e-08, 8.626e-08, 7.652e-08, 8.539e-08),
    "bf16-csr-3run-64x128": (1.080e-03, 8.382e-04, 1.859e-07, 6.342e-08, 5.079e-08, 1.055e-07, 6.030e-08, 1.488e-07, 6.052e-08, 8.684e-08),
    "bf16x-shuffled-3run-64x128": (1.073e-07, 2.007e-07, 2.963e-07, 6.486e-08, 2.913e-08, 1.090e-07, 3.426e-08, 1.715e-07, 5.443e-08, 1.044e-07),
    "f32-shuffled-3run-32x64": (1.049e-07, 1.264e-06, 1.721e-06, 9.095e-08, 4.191e-08, 9.484e-07, 5.354e-08, 1.103e-06, 4.743e-08, 1.196e-06),
}

CASES = [(mode, order, graphs, 64, 128) for mode in (1, 3) for order in ("shuffled", "csr") for graphs in (1, 3)]
CASES += [(3 | H.X_BF16, "shuffled", 3, 64, 128), (1, "shuffled", 3, 32, 64)]


def case_id(c):
    mode, order, graphs, K, N = c
    name = {1: "f32", 3: "bf16", 3 | H.X_BF16: "bf16x"}[mode]
    return f"{name}-{order}-{graphs}run-{K}x{N}"


def test_recorded_errors_are_sane():
    for key, v in PARENT_ERR.items():
        assert len(v) == len(H.QUANTITIES)
        assert v[0] < (1e-5 if key.startswith("f32") else 2e-2), key
    assert set(PARENT_ERR) == {case_id(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_at_level_size_matches_the_f64_reference(case):
    mode, order, graphs, K, N = case
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(23)
    c = H.build(g, ROWS, SEGS, K, N, dev, order, graphs, giant=GIANT, in16=bool(mode & H.X_BF16))
    assert int(c.pb.rowptr[c.giant_seg + 1] - c.pb.rowptr[c.giant_seg]) == GIANT
    assert _lib.lib.spt_fused_linear_pool_supported(K, N, mode)
    o = H.call_forward(c, mode)
    # the same call without `arg`, and once more as it was: bitwise the same
    o2 = H.call_forward(c, mode, want_arg=False)
    o3 = H.call_forward(c, mode)
    for other in (o2, o3):
        assert other.status == 0
        for f in ("out", "raw", "argpos"):
            assert torch.equal(getattr(other, f).view(torch.int32), getattr(o, f).view(torch.int32)), f
    assert bool((o2.arg == -1).all()) and torch.equal(o3.arg, o.arg)
    del o2, o3
    parent = PARENT_ERR.get(case_id(case))
    H.check_forward(c, mode, o, case_id(case), parent=None if parent is None else dict(zip(H.QUANTITIES, parent)))
    assert parent is not None, "no recorded error of the parent commit for this case"


@pytest.mark.gpu
def test_bf16_storage_is_refused_outside_the_bf16_mode():
    """x held as bf16 exists for matrix mode 3 only: with the f32 mode word the entry has to say so
    (an error status, nothing launched, no output touched) instead of reading x as something else."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    c = H.build(g, 40_000, 1000, 64, 128, dev, "shuffled", 1, in16=True)
    o = H.call_forward(c, 1 | H.X_BF16)
    assert o.status != 0
    assert bool(torch.isnan(o.out).all()) and bool(torch.isnan(o.raw).all()) and bool((o.argpos == -1).all())
    ok = H.call_forward(c, 3 | H.X_BF16)
    assert ok.status == 0 and bool(torch.isfinite(ok.out).all())
