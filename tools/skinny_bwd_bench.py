"""Time the backward of the attention blocks' Linears (K = 64 -> N = 192 qkv, 64 -> 64 out_proj) at the
scene-S level sizes through the C ABI: the one-pass entry (spt_skinny_linear_bwd_m_f32: gx, gW, gb from
one read of gy and x) against the two-launch route (spt_skinny_linear_wt_m_f32 + spt_skinny_dw_pre_m_f32).
    python tools/skinny_bwd_bench.py [--rows 428571 178571] [--mode 1] [--reps 20] [--pre]
ms per call and GB/s over the bytes each route has to move, every operand counted once per launch that
reads or writes it: one-pass (N + 2 K) 4 B per row, two-launch 2 (N + K) 4 B per row."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from superpoint_transformer_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[428_571, 178_571])
ap.add_argument("--mode", type=int, default=1, help="1 split bf16 (default), 3 bf16")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--pre", action="store_true", help="with the folded pre-norm's tables (one graph)")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
P, L = _lib.ptr, _lib.lib
K = 64


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / a.reps)
    return best


for rows in a.rows:
    for N in (192, 64):
        gy = torch.randn(rows, N, device=dev, generator=g)
        x = torch.randn(rows, K, device=dev, generator=g)
        W = torch.randn(N, K, device=dev, generator=g) * 0.1
        tabs = [torch.rand(1, K, device=dev, generator=g) + 0.5 for _ in range(2)] + \
               [torch.rand(K, device=dev, generator=g)] if a.pre else [None, None, None]
        gx, gw, gb = torch.empty(rows, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        gx2, gw2, gb2 = torch.empty_like(gx), torch.empty_like(gw), torch.empty_like(gb)
        ws = torch.empty(max(L.spt_skinny_linear_bwd_workspace_bytes(K, N), L.spt_skinny_dw_workspace_bytes(K, N)),
                         dtype=torch.uint8, device=dev)
        s = _lib.stream_ptr(dev)

        def one_pass():
            _lib.check(L.spt_skinny_linear_bwd_m_f32(P(gy), P(x), P(W), rows, N, K, P(gx), P(gw), P(gb), P(tabs[0]),
                                                     P(tabs[1]), P(tabs[2]), None, 1, a.mode, P(ws), ws.numel(), s),
                       "spt_skinny_linear_bwd_m_f32")

        def two_launch():
            _lib.check(L.spt_skinny_linear_wt_m_f32(P(gy), rows, N, P(W), K, P(gx2), a.mode, s),
                       "spt_skinny_linear_wt_m_f32")
            _lib.check(L.spt_skinny_dw_pre_m_f32(P(gy), P(x), rows, N, K, P(gw2), P(gb2), P(tabs[0]), P(tabs[1]),
                                                 P(tabs[2]), None, 1, a.mode, P(ws), ws.numel(), s),
                       "spt_skinny_dw_pre_m_f32")

        t1, t2 = timed(one_pass), timed(two_launch)
        b1, b2 = rows * (N + 2 * K) * 4, rows * 2 * (N + K) * 4
        same = torch.equal(gx, gx2)
        dw = ((gw - gw2).abs().max() / gw2.abs().max()).item()
        print(f"rows {rows:7d} {K}->{N:3d} mode {a.mode}{' pre' if a.pre else ''}: one-pass {t1:.4f} ms "
              f"{b1 / t1 / 1e6:7.0f} GB/s | two-launch {t2:.4f} ms {b2 / t2 / 1e6:7.0f} GB/s | "
              f"x{t2 / t1:.2f}  gx bitwise {same}  gW rel diff {dw:.1e}")
