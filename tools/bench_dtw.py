#!/usr/bin/env python3
"""Stage-5 timings on the GPU (profiles/r29_notes.md): jatts_dtw alone at (N, M) = (800, 800) and (2000, 1800) for batches of 1 and of 64
pairs (ms per launch, pairs per second), then a 100-utterance synthetic set through Evaluator.evaluate_batch with the stage shares from
hip.profile_begin / profile_end.  There is no speed gate: nothing in the package computed this before.

    python tools/bench_dtw.py [--json PATH] [--reps 5] [--utterances 100]
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from jatts_amd import hip  # noqa: E402
from jatts_amd.evaluate import Evaluator  # noqa: E402


def time_dtw(n, m, pairs, reps, dev):
    geo = hip.PairGeometry([n] * pairs, [m] * pairs)
    cost = torch.rand(geo.c_total, device=dev) + 0.01
    bufs = (torch.empty(geo.d_total, dtype=torch.int32, device=dev), torch.empty(geo.p_total, dtype=torch.int32, device=dev),
            torch.empty(geo.p_total, dtype=torch.int32, device=dev), torch.empty(pairs, dtype=torch.int32, device=dev),
            torch.empty(pairs, dtype=torch.float64, device=dev))
    hip.dtw(geo, cost, bufs)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip.dtw(geo, cost, bufs)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    return {"n": n, "m": m, "pairs": pairs, "ms_per_launch": med, "ms_min": float(min(ms)), "pairs_per_s": pairs / med * 1e3,
            "cells_per_us": pairs * n * m / med * 1e-3}


def synthetic_wave(fs, seconds, f_start, f_end, seed):
    n = int(seconds * fs)
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    phase = 2.0 * np.pi * np.cumsum(f_start + (f_end - f_start) * t / seconds) / fs
    x = sum(0.8 ** h * np.sin(h * phase + rng.uniform(0, 6.28)) for h in range(1, 20))
    x *= (0.55 + 0.45 * np.sin(2.0 * np.pi * 2.3 * t)) * 0.5 / np.abs(x).max()
    return x.astype(np.float32)


def time_set(n_utts, batch, dev, fs=24000):
    rng = np.random.default_rng(0)
    items = []
    for k in range(n_utts):
        sec = float(rng.uniform(2.0, 6.0))
        f = float(rng.uniform(100.0, 180.0))
        items.append((synthetic_wave(fs, sec, f, f * 1.3, k), synthetic_wave(fs, sec * float(rng.uniform(0.9, 1.1)), f, f * 1.4, 1000 + k), f"utt{k}"))
    items.sort(key=lambda it: it[0].size)
    ev = Evaluator(dev)
    ev.evaluate_batch(items[:2], fs, 70.0, 400.0)      # tables, workspace
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, n_utts, batch):
        ev.evaluate_batch(items[i:i + batch], fs, 70.0, 400.0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    hip.profile_begin()
    for i in range(0, n_utts, batch):
        ev.evaluate_batch(items[i:i + batch], fs, 70.0, 400.0)
    share = collections.defaultdict(float)
    for tag, _, ms in hip.profile_end():
        share[tag] += ms
    audio = sum(it[0].size + it[1].size for it in items) / fs
    return {"utterances": n_utts, "batch": batch, "audio_seconds": audio, "wall_s": wall, "utterances_per_s": n_utts / wall,
            "timed_stage_ms": dict(share), "untimed": "conv1d = the mel projection and the DCT; the STFT, log, autocorrelation and pitch-pick launches carry no profile tag"}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--json", default=None)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--utterances", type=int, default=100)
    p.add_argument("--batch-size", type=int, default=16)
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    out = {"dtw": [time_dtw(n, m, pairs, args.reps, dev) for n, m in ((800, 800), (2000, 1800)) for pairs in (1, 64)],
           "set": time_set(args.utterances, args.batch_size, dev)}
    for r in out["dtw"]:
        print(f"dtw {r['n']} x {r['m']} x {r['pairs']:2d} pairs: {r['ms_per_launch']:.3f} ms per launch, {r['pairs_per_s']:.1f} pairs/s, "
              f"{r['cells_per_us']:.1f} cells/us")
    s = out["set"]
    print(f"set of {s['utterances']} pairs ({s['audio_seconds']:.0f} s of audio, batches of {s['batch']}): {s['wall_s']:.3f} s, "
          f"{s['utterances_per_s']:.1f} pairs/s; tagged stages (ms): " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(s["timed_stage_ms"].items())))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
