#!/usr/bin/env python3
"""Times the sample-rate converter at stage-1 batch geometries: 64 utterances x 5 s at 48 -> 24 kHz and at 44.1 -> 24 kHz.

  leg A  jatts_resample (jatts_amd/csrc/resample.hip): the exact-f32 MFMA contraction over blocks of outputs, kernel launch only
         (output buffer allocated once).
  leg B  the torch.nn.functional.conv1d polyphase composition (the torchaudio formulation, f32): the waveforms as a (B, 1, n) batch, the
         taps as `up` kernels of one phase each, stride `down`, then a transpose to interleave the phases.  Same taps, same zero
         padding; for TIMING only -- the product path carries no torch arithmetic.

Both legs start from the same samples on the device and are timed with device events around `--iters` back-to-back calls, after
`--warmup` calls each; the legs alternate `--reps` times and the table gives median and min .. max over the repetitions.  Shares of
the 157.3 TFLOP/s f32 MFMA peak, of leg A: USEFUL = 2 x (taps per output) x outputs over the time, ISSUED = 2 x K x Nbp x blocks over
the time (the MFMA work including the table's zero rows and padding columns).  End-to-end figures of one launch each, not a
profiler's kernel time.  The two legs' outputs are compared once.  Prints a table and one JSON line per geometry; needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as tf

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jatts_amd import features, hip  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def polyphase_kernels(taps, up, down):
    """(up, 1, k1) conv1d weight and the left padding: phase c of output block q reads x[q * down - L + i] * taps[c * down - (i - L) * up + half_len]."""
    half_len = taps.size // 2
    lead = half_len // up
    k1 = ((up - 1) * down + half_len) // up + lead + 1
    i = np.arange(k1, dtype=np.int64)[None, :]
    c = np.arange(up, dtype=np.int64)[:, None]
    j = c * down - (i - lead) * up + half_len
    ok = (j >= 0) & (j < taps.size)
    return np.where(ok, taps[np.clip(j, 0, taps.size - 1)], np.float32(0)).astype(np.float32)[:, None, :], lead


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def bench(dev, sr_in, sr_out, utts, seconds, iters, warmup, reps):
    rs = features.Resampler(dev, sr_in, sr_out)
    g, up, down = rs.geometry, rs.up, rs.down
    n = int(seconds * sr_in)
    gen = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(utts * n, generator=gen)).to(dev)
    pw = features.PackedWaves(x, [n] * utts)
    n_out = rs.out_len(n)
    cu_out = hip.h2d([i * n_out for i in range(utts + 1)], torch.int32, dev)
    out = torch.empty(utts * n_out, dtype=torch.float32, device=dev)

    def leg_a():
        return hip.resample(pw.cu, cu_out, pw.lens, [n_out] * utts, pw.x, rs.table, up, down, rs.half_len, out=out)

    w, lead = polyphase_kernels(rs.taps.cpu().numpy(), up, down)
    wt = torch.from_numpy(w).to(dev)
    blocks1 = -(-n_out // up)
    right = max(0, (blocks1 - 1) * down + w.shape[2] - lead - n)
    xb = x.view(utts, 1, n)

    def leg_b():
        y = tf.conv1d(tf.pad(xb, (lead, right)), wt, stride=down)              # (B, up, blocks)
        return y.transpose(1, 2).reshape(utts, -1)[:, :n_out]

    ya = leg_a().view(utts, n_out).clone()
    yb = leg_b()
    diff = float((ya - yb).abs().max())
    for _ in range(warmup):
        leg_a()
        leg_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(leg_a, iters))
        tb.append(timed(leg_b, iters))
    taps_per_out = (2 * rs.half_len + 1) / up
    useful = 2.0 * taps_per_out * utts * n_out
    issued = 2.0 * g["K"] * g["Nbp"] * utts * (-(-n_out // g["Nb"]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    res = dict(sr_in=sr_in, sr_out=sr_out, utts=utts, seconds=seconds, K=g["K"], Nb=g["Nb"], Nbp=g["Nbp"],
               resample_ms=dict(median=ma * 1e3, min=min(ta) * 1e3, max=max(ta) * 1e3),
               conv1d_ms=dict(median=mb * 1e3, min=min(tb) * 1e3, max=max(tb) * 1e3),
               useful_share_of_peak=useful / ma / PEAK_F32_MFMA, issued_share_of_peak=issued / ma / PEAK_F32_MFMA,
               useful_over_issued=useful / issued, speedup_over_conv1d=mb / ma, max_abs_diff_between_legs=diff)
    print(f"{sr_in} -> {sr_out} Hz, {utts} x {seconds} s (K {g['K']}, Nb {g['Nb']} / Nbp {g['Nbp']}; {iters} calls per window, {reps} alternating windows)")
    print(f"  jatts_resample          {ma * 1e3:8.3f} ms  ({min(ta) * 1e3:.3f} .. {max(ta) * 1e3:.3f})   useful {100 * res['useful_share_of_peak']:.1f} % "
          f"issued {100 * res['issued_share_of_peak']:.1f} % of 157.3 TFLOP/s")
    print(f"  conv1d polyphase (f32)  {mb * 1e3:8.3f} ms  ({min(tb) * 1e3:.3f} .. {max(tb) * 1e3:.3f})   ratio {mb / ma:.2f} x   max |a - b| {diff:.2e}")
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: no GPU visible (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    for sr_in, sr_out in ((48000, 24000), (44100, 24000)):
        bench(dev, sr_in, sr_out, a.utts, a.seconds, a.iters, a.warmup, a.reps)


if __name__ == "__main__":
    main()
