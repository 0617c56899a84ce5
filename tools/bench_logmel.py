#!/usr/bin/env python3
"""Times the STFT of the feature extractor at the bench batch geometry: 64 utterances x 230 400 samples at 24 kHz, n_fft 2048, hop 300
(769 frames each).

  leg A  jatts_stft_mag: frames from the waveform inside the kernel, magnitude out (jatts_amd/features/stft.py).
  leg B  the entry points FbankFrontEnd composes, at n_fft 2048: jatts_frame_signal -> jatts_conv1d (DFT as a k = 1 conv, exact f32)
         -> jatts_power_spectrum.  Zero padding and a power spectrum: for TIMING and footprint only.

Both legs start from the same samples on the device and are timed with device events around `--iters` back-to-back calls, after
`--warmup` calls each; the legs alternate `--reps` times and the table gives median and min .. max over the repetitions.  The share of
peak is the useful work 2 x n_fft x 2 x n_bins x frames over the time and over the 157.3 TFLOP/s f32 MFMA peak: an end-to-end figure of
each leg (leg B's includes its two row-wise launches).  Peak memory is torch's allocator peak above what is live before the leg (samples,
tables).  Interior frames (no padding involved) of the two legs are compared once.  Prints a table and one JSON line; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jatts_amd import features, hip  # noqa: E402
from jatts_amd._abi import F32  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--samples", type=int, default=230400)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="also time the whole log-mel call (upload, STFT, mel projection, log)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logmel: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    sr, n_fft, hop = 24000, 2048, 300
    ex = features.LogMelExtractor(dev, sr, fft_size=n_fft, hop_size=hop, win_length=n_fft, num_mels=80, fmin=80, fmax=7600)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(a.samples, dtype=torch.float64) / sr
    waves = [(0.5 * torch.sin(2 * np.pi * (110.0 + 3.0 * i) * t) * torch.sin(2 * np.pi * 1.3 * t) ** 2).float()
             + 1e-3 * torch.randn(a.samples, generator=g) for i in range(a.utts)]
    ns = [a.samples] * a.utts
    rb = hip.RaggedBatch([features.frame_count(n, n_fft, hop) for n in ns], dev)
    x = torch.cat(waves).to(dev)
    cu = hip.h2d([i * a.samples for i in range(a.utts + 1)], torch.int32, dev)
    n_bins = n_fft // 2 + 1
    flops = 2.0 * n_fft * 2 * n_bins * rb.total

    # leg B's constants, as FbankFrontEnd lays them out
    nbp = hip.round_up(n_bins, 8)
    win = torch.from_numpy(features.padded_window("hann", None, n_fft)).float().to(dev)
    n = torch.arange(n_fft, dtype=torch.float64)
    k = torch.arange(n_bins, dtype=torch.float64)
    ang = 2.0 * np.pi * k.unsqueeze(1) * n.unsqueeze(0) / n_fft
    w = torch.zeros(2 * nbp, n_fft, dtype=torch.float64)
    w[:n_bins] = torch.cos(ang)
    w[nbp:nbp + n_bins] = -torch.sin(ang)
    dft = hip.pack_conv_weight(w.float().unsqueeze(-1).to(dev), F32, 64)
    ldp = hip.round_up(nbp, 64)
    del w, ang

    def leg_a():
        return hip.stft_mag(rb, cu, ns, x, ex.stft.table, n_fft, hop, ex.stft.ld_mag)[0]

    def leg_b():
        frames = hip.frame_signal(rb, cu, x, win, n_fft, hop, n_fft)
        spec = hip.conv1d(rb, frames, dft, n_fft, 2 * nbp, 1, dtype=F32)
        return hip.power_spectrum(spec, nbp, ldp)

    def leg_full():
        return ex(waves)[1]

    legs = {"A stft_mag": leg_a, "B frame+dft+power": leg_b}
    if a.full:
        legs["A whole log-mel call"] = leg_full

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    peak = {}
    for name, fn in legs.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del out
    # interior frames see no padding: magnitude^2 of leg A against the power of leg B
    T = rb.lens[0]
    inner = [t_ for t_ in range(T) if t_ * hop - n_fft // 2 >= 0 and t_ * hop + n_fft // 2 <= a.samples]
    ma, pb = leg_a()[inner, :n_bins].double(), leg_b()[inner, :n_bins].double()
    diff = float(((ma * ma - pb).abs().amax(dim=1) / pb.amax(dim=1)).max())
    del ma, pb
    ms = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    res = {"geometry": f"{a.utts} x {a.samples} samples, n_fft {n_fft}, hop {hop}, {rb.total} frames", "useful_gflop": flops / 1e9,
           "interior_power_rel_diff": diff, "legs": {}}
    print(f"{res['geometry']}; {flops / 1e9:.1f} useful GFLOP; interior frames, A^2 against B (relative to the frame's maximum): {diff:.2e}")
    print(f"{'leg':24s} {'ms median':>10s} {'min':>8s} {'max':>8s} {'of f32 MFMA peak':>17s} {'peak MiB':>10s}")
    for name in legs:
        v = ms[name]
        med = statistics.median(v)
        share = flops / (med * 1e-3) / PEAK_F32_MFMA
        res["legs"][name] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "share_of_f32_mfma_peak": share, "peak_mib": peak[name]}
        print(f"{name:24s} {med:10.3f} {min(v):8.3f} {max(v):8.3f} {share:17.3f} {peak[name]:10.1f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
