#!/usr/bin/env python3
"""Micro-benchmark of the conv weight gradient: the exact-f32 jatts_conv1d_wgrad (v_mfma_f32_32x32x2_f32) beside the emulated jatts_conv1d_wgrad_emul
(JATTS_F32E on v_mfma_f32_16x16x32_bf16), both split-K over the sequences.  HIP events on the launch stream, warm-up, median of --reps runs of --inner
launches each, and the spread (max - min) / median of those runs; shapes: the FastSpeech2 JSUT training step's (tools/conv_shapes.py --train fs2) plus the
round 3 list.
    python tools/bench_wgrad.py [--reps 7] [--inner 10] [--batch 32] [--frames 768]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from jatts_amd import hip  # noqa: E402

# (n_out, c_in, k)
SHAPES = [(1536, 384, 3), (384, 1536, 3), (384, 384, 1), (768, 384, 1), (1152, 384, 1), (256, 384, 3), (256, 256, 3), (80, 384, 1),
          (384, 192, 5), (384, 192, 3), (384, 192, 1), (512, 512, 3), (2048, 512, 1), (512, 512, 5)]


def timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / inner)
    med = statistics.median(runs)
    return med, (max(runs) - min(runs)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=768)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T = a.batch, a.frames
    rb = hip.RaggedBatch([T] * B, dev)
    probe = hip.mfma_ceiling(hip.F32E, device=dev)
    print(f"# batch {B} x {T} frames; bf16 MFMA probe of this box: {probe}")
    print("#   n_out  c_in k |  f32 us  TFLOP/s spread | emul us  TFLOP/s spread | f32 / emul")
    for n, c, k in SHAPES:
        x = torch.randn(B * T, c, device=dev)
        dy = torch.randn(B * T, n, device=dev)
        fl = 2.0 * B * T * n * c * k
        tf, sf = timed(lambda: hip.conv1d_wgrad(rb, x, dy, c, n, k, 1, (k - 1) // 2), a.reps, a.inner)
        te, se = timed(lambda: hip.conv1d_wgrad(rb, x, dy, c, n, k, 1, (k - 1) // 2, dtype=hip.F32E), a.reps, a.inner)
        print(f"wgrad {n:5d} {c:5d} {k} | {tf:7.1f} {fl / tf / 1e6:7.1f} {sf * 100:5.1f}% | {te:7.1f} {fl / te / 1e6:7.1f} {se * 100:5.1f}% | {tf / te:5.2f}")


if __name__ == "__main__":
    main()
