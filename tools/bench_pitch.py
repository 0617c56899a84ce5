#!/usr/bin/env python3
"""Times the pitch extractor at the bench batch geometry: 64 utterances x 768 frames at 24 kHz, n_fft 2048, hop 300,
f0 range 70-400 Hz.

  legs   jatts_stft_mag (the pitch window's table), jatts_acf_from_mag, jatts_pitch_pick, jatts_f0_continuous_log, each alone on the
         previous one's output, and the four in a row ("raw + continuous log").
  yard   the same definition composed from torch: reflect padding, unfold, window, torch.fft.rfft, |.|^2, torch.fft.irfft, the window
         correction, candidates, parabolic peak, octave cost, argmax, voicing.  float32, for TIMING only (its sums have another order).

Everything starts from the same samples on the device and is timed with device events around `--iters` back-to-back calls, after `--warmup`
calls each; the legs alternate `--reps` times and the table gives median and min .. max over the repetitions.  The MFMA share of
jatts_acf_from_mag is its multiply-adds, 2 x K x Lp x frames (padding included: the kernel runs them), over its time and over the
157.3 TFLOP/s f32 MFMA peak.  Voicing decisions and f0 of the two sides are compared once.  Prints a table and one JSON line; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jatts_amd import features, hip  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    sr, n_fft, hop, f0min, f0max = 24000, 2048, 300, 70, 400
    samples = (a.frames - 1) * hop
    ex = features.Pitch(fs=sr, n_fft=n_fft, hop_length=hop, use_token_averaged_f0=False, device=dev)
    lo, hi, sum_w2, front, acf = ex.tables(f0min, f0max)
    w_len = features.pitch_geometry(sr, n_fft, f0min, f0max)[2]
    g = torch.Generator().manual_seed(0)
    t = torch.arange(samples, dtype=torch.float64) / sr
    waves = []
    for i in range(a.utts):
        f = 110.0 + 3.0 * i + 40.0 * t
        ph = 2 * np.pi * torch.cumsum(f, 0) / sr
        x = sum(0.8 ** h * torch.sin(h * ph) for h in range(1, 9)) * (torch.sin(2 * np.pi * 0.7 * t) > -0.6)
        waves.append((0.5 * x / x.abs().max()).float() + 1e-3 * torch.randn(samples, generator=g))
    pw = features.PackedWaves.from_list(waves, dev)
    rb = hip.RaggedBatch([features.frame_count(n, n_fft, hop) for n in pw.lens], dev)
    assert rb.lens == [a.frames] * a.utts
    peak = hip.wave_gain_peak(pw.cu, a.utts, pw.x, 1.0)

    def stft():
        return front.magnitude(pw)[1]
    mag = stft()
    r = hip.acf_from_mag(rb, mag, acf)
    f0, _ = hip.pitch_pick(rb, r, peak, 2, lo, hi, sr, f0min, sum_w2)

    def whole():
        m = stft()
        rr = hip.acf_from_mag(rb, m, acf)
        ff, _ = hip.pitch_pick(rb, rr, peak, 2, lo, hi, sr, f0min, sum_w2)
        return hip.f0_continuous_log(rb, ff)

    win = torch.from_numpy(features.padded_window("hann", w_len, n_fft)).float().to(dev)
    rw = torch.from_numpy(features.window_autocorrelation(win.double().cpu().numpy(), hi + 2))
    corr = (rw[0] / rw).float().to(dev)
    xb = pw.x.view(a.utts, samples)
    taus = torch.arange(lo, hi + 1, device=dev, dtype=torch.float32)

    def yard():
        fr = torch.nn.functional.pad(xb.unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect").squeeze(1).unfold(1, n_fft, hop) * win
        rr = torch.fft.irfft(torch.fft.rfft(fr, dim=-1).abs() ** 2, n=n_fft, dim=-1)[..., :hi + 2]
        rho = rr / rr[..., :1].clamp_min(1e-30) * corr
        p, q, s = rho[..., lo - 1:hi], rho[..., lo:hi + 1], rho[..., lo + 1:hi + 2]
        cand = (q >= p) & (q > s)
        den = p - 2 * q + s
        off = torch.where(den < 0, (0.5 * (p - s) / den).clamp(-0.5, 0.5), torch.zeros_like(den))
        pk = q - 0.25 * (p - s) * off
        score = torch.where(cand, pk - 0.01 * torch.log2((taus + off) * f0min / sr), torch.full_like(pk, -float("inf")))
        best = score.argmax(dim=-1, keepdim=True)
        level = (rr[..., 0] / sum_w2).sqrt()
        voiced = cand.any(-1) & (pk.gather(-1, best).squeeze(-1) >= 0.45) & (level >= 0.03 * xb.abs().amax(dim=1, keepdim=True))
        return torch.where(voiced, sr / (best.squeeze(-1) + lo + off.gather(-1, best).squeeze(-1)), torch.zeros_like(level))

    legs = {"jatts_stft_mag": stft, "jatts_acf_from_mag": lambda: hip.acf_from_mag(rb, mag, acf),
            "jatts_pitch_pick": lambda: hip.pitch_pick(rb, r, peak, 2, lo, hi, sr, f0min, sum_w2),
            "jatts_f0_continuous_log": lambda: hip.f0_continuous_log(rb, f0), "raw + continuous log": whole, "torch.fft yardstick": yard}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ours, theirs = f0.view(a.utts, a.frames).double(), yard().double()
    both = (ours > 0) & (theirs > 0)
    agree = float(((ours > 0) == (theirs > 0)).double().mean())
    cents = float((1200.0 * torch.log2(ours[both] / theirs[both]).abs()).median()) if both.any() else float("nan")
    ms = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    flops = 2.0 * acf.shape[0] * acf.shape[1] * rb.total
    res = {"geometry": f"{a.utts} x {a.frames} frames, {sr} Hz, n_fft {n_fft}, hop {hop}, f0 {f0min}-{f0max} Hz (lags {lo}..{hi}, window {w_len})",
           "voicing_agreement_with_yardstick": agree, "median_cents_against_yardstick": cents, "legs": {}}
    print(res["geometry"])
    print(f"voicing agrees with the yardstick on {agree:.4f} of the frames; median |f0 difference| where both are voiced: {cents:.2e} cents")
    print(f"{'leg':26s} {'ms median':>10s} {'min':>8s} {'max':>8s}")
    for name in legs:
        v = ms[name]
        res["legs"][name] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
        print(f"{name:26s} {statistics.median(v):10.3f} {min(v):8.3f} {max(v):8.3f}")
    share = flops / (res["legs"]["jatts_acf_from_mag"]["ms_median"] * 1e-3) / PEAK_F32_MFMA
    res["acf_from_mag_gflop"], res["acf_from_mag_share_of_f32_mfma_peak"] = flops / 1e9, share
    print(f"jatts_acf_from_mag: {flops / 1e9:.1f} GFLOP in its table's shape ({acf.shape[0]} x {acf.shape[1]}), {share:.3f} of the f32 MFMA peak")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
