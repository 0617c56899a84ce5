#!/usr/bin/env python3
"""Times Griffin-Lim at decode batch geometry: 64 utterances x 768 frames, n_iter = 64, at (n_fft, hop) = (2048, 300) and (1024, 256).

  leg A  jatts_amd.vocoder.GriffinLim: one jatts_gl_istft and one jatts_gl_stft_project launch per iteration over the whole batch (the
         exact-f32 MFMA contractions of csrc/griffinlim.hip), scratch allocated once per call.
  leg B  a torch composition of the SAME definition on the same GPU: torch.stft(center=True, pad_mode="constant") / torch.istft in
         complex64 over the (B, samples) batch, the projection in torch ops.  For TIMING only -- the product path carries no torch
         arithmetic.

Both legs start from the same magnitudes and initial phases on the device; each call is timed with device events around the synchronised
call, after `--warmup` calls each (tables, code objects, FFT plans); the legs alternate `--pairs` times and the table gives median and
min .. max over the pairs.  TFLOP/s of leg A: the operations of the two contractions as issued, per frame and iteration
2 n_fft (2 nbp) for the STFT and 2 (J 2 nbp) hopp for the span ISTFT (plus the final ISTFT), over the call's time -- an end-to-end rate over
the 157.3 TFLOP/s f32 MFMA peak, not a profiler's kernel share.  The two legs' waveforms are compared once after 2 iterations (the loop
is chaotic after 64).  Prints a table and one JSON line per geometry; needs the GPU."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jatts_amd import hip  # noqa: E402
from jatts_amd.vocoder import GriffinLim  # noqa: E402

PEAK_F32_MFMA = 157.3e12
TINY = 2.0 ** -126


def torch_griffin_lim(S, P0, w, n_fft, hop, n_iter, beta):
    """S, P0: (B, T, n_bins) -> (B, (T - 1) * hop)"""
    L = (S.shape[1] - 1) * hop
    inv = lambda X: torch.istft(X.transpose(1, 2), n_fft, hop, n_fft, window=w, center=True, length=L)      # noqa: E731
    X = S * P0
    c_prev = torch.zeros_like(X)
    for _ in range(n_iter):
        C = torch.stft(inv(X), n_fft, hop, n_fft, window=w, center=True, pad_mode="constant", return_complex=True).transpose(1, 2)
        A = C - beta * c_prev
        X, c_prev = S * A / (A.abs() + TINY), C
    return inv(X)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def bench(dev, n_fft, hop, utts, frames, n_iter, warmup, pairs):
    gl = GriffinLim(dev, n_fft, hop, n_iter=n_iter)
    w = torch.from_numpy(gl.window).float().to(dev)
    L = (frames - 1) * hop
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    t = torch.arange(L, device=dev, dtype=torch.float32)
    x = 0.3 * torch.sin(2 * math.pi * 0.031 * t + 3.0 * torch.sin(2 * math.pi * 0.0007 * t)) + 0.02 * torch.randn(utts, L, generator=gen, device=dev)
    S3 = torch.stft(x, n_fft, hop, n_fft, window=w, center=True, pad_mode="constant", return_complex=True).transpose(1, 2).abs().contiguous()
    assert S3.shape == (utts, frames, gl.n_bins)
    rb = hip.RaggedBatch([frames] * utts, dev)
    S = torch.zeros(rb.total, gl.nbp, dtype=torch.float32, device=dev)
    S[:, :gl.n_bins] = S3.reshape(rb.total, gl.n_bins)
    P0 = gl.initial_phases(rb.total, 0)
    P3 = P0.view(utts, frames, gl.n_bins)

    def leg_a(n=None):
        return gl.run(rb, S, init=P0, n_iter=n)

    def leg_b(n=n_iter):
        return torch_griffin_lim(S3, P3, w, n_fft, hop, n, gl.beta)

    ya, yb = leg_a(2)[:utts * L].view(utts, L), leg_b(2)
    diff = float((ya - yb).abs().max())
    for _ in range(warmup):
        leg_a()
        leg_b()
    ta, tb = [], []
    for _ in range(pairs):
        ta.append(timed(leg_a))
        tb.append(timed(leg_b))
    hopp, J = hip.round_up(hop, 32), gl.J
    stft_flop, istft_flop = 2.0 * n_fft * 2 * gl.nbp, 2.0 * J * 2 * gl.nbp * hopp
    flop = rb.total * (n_iter * (stft_flop + istft_flop) + istft_flop)
    ma, mb = statistics.median(ta), statistics.median(tb)
    res = dict(n_fft=n_fft, hop=hop, utts=utts, frames=frames, n_iter=n_iter, pairs=pairs,
               griffin_lim_s=dict(median=ma, min=min(ta), max=max(ta)), torch_s=dict(median=mb, min=min(tb), max=max(tb)),
               mflop_per_frame_iteration=dict(stft=stft_flop * 1e-6, istft=istft_flop * 1e-6), tflop=flop * 1e-12,
               tflops=flop / ma * 1e-12, share_of_f32_mfma_peak=flop / ma / PEAK_F32_MFMA, torch_over_griffin_lim=mb / ma,
               max_abs_diff_after_2_iterations=diff)
    print(f"n_fft {n_fft}, hop {hop}: {utts} x {frames} frames, {n_iter} iterations ({pairs} alternating pairs)")
    print(f"  jatts GriffinLim       {ma:8.4f} s / batch  ({min(ta):.4f} .. {max(ta):.4f})   {res['tflops']:.1f} TFLOP/s issued, "
          f"{100 * res['share_of_f32_mfma_peak']:.1f} % of 157.3 TFLOP/s")
    print(f"  torch.stft / istft c64 {mb:8.4f} s / batch  ({min(tb):.4f} .. {max(tb):.4f})   torch / jatts {mb / ma:.2f} x   "
          f"max |a - b| after 2 iterations {diff:.2e}")
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_griffin_lim: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    for n_fft, hop in ((2048, 300), (1024, 256)):
        bench(dev, n_fft, hop, a.utts, a.frames, a.iters, a.warmup, a.pairs)


if __name__ == "__main__":
    main()
