#!/usr/bin/env python3
"""CPU emulation of the summation orders jatts_stft_mag could use, on the signals of tests/golden/logmel_kat.npz (no GPU, ~10 s per order).

The f32 MFMA is a k-ordered fmaf chain, so its result is a function of the order of the sum alone and numpy can restate it: a float32
accumulator, products exact in float64 (24 x 24 bits), one rounding per term.  Prints the three error measures of the GPU test for each
order as multiples of the float32-FFT yardstick E32 stored in the fixture (the table of profiles/r15_notes.md):

  --accs P     P accumulators taking alternate 16-sample steps, added pairwise at the end (P = 1: one chain)
  --chunk C    a chain of its own per C samples, started at zero, chunks added in order (what the kernel does with C = 64)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from jatts_amd import features as F  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_logmel", os.path.join(ROOT, "tests", "golden", "make_golden_logmel.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def chain(A, B, accs=1):
    """A (M, K) f32 x B (K, N) f32 in the kernel's k order: step s, MFMA j takes k = 16 s + j and 16 s + 8 + j."""
    acc = [np.zeros((A.shape[0], B.shape[1]), dtype=np.float32) for _ in range(accs)]
    for s in range(A.shape[1] // 16):
        for j in range(8):
            for k in (16 * s + j, 16 * s + 8 + j):
                acc[s % accs] = (acc[s % accs].astype(np.float64) + A[:, k:k + 1].astype(np.float64) * B[k:k + 1].astype(np.float64)).astype(np.float32)
    while len(acc) > 1:
        acc = [acc[i] + acc[i + 1] for i in range(0, len(acc), 2)]
    return acc[0]


def chunked(A, B, chunk, accs):
    if not chunk:
        return chain(A, B, accs)
    total = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k0 in range(0, A.shape[1], chunk):
        total = total + chain(A[:, k0:k0 + chunk], B[k0:k0 + chunk])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accs", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=0)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "logmel_kat.npz"))
    for name, s in gen.SETTINGS.items():
        n_fft, hop = s["fft_size"], s["hop_size"]
        nb = n_fft // 2 + 1
        nbp = (nb + 31) // 32 * 32
        table = F.dft_table(F.padded_window("hann", s["win_length"], n_fft), n_fft)
        off, mags, pows = 0, [], []
        for L in (int(v) for v in z[f"{name}_lens"]):
            x = z[f"{name}_wave"][off:off + L]
            off += L
            spec = chunked(x[F.frame_indices(L, n_fft, hop)], table, a.chunk, a.accs)
            re, im = spec[:, :nb].astype(np.float64), spec[:, nbp:nbp + nb].astype(np.float64)
            p = (re * re + im * im).astype(np.float32)
            mags.append(np.sqrt(p))
            pows.append(p.sum(axis=1, dtype=np.float32))
        mag = np.concatenate(mags)
        K = (nb + 63) // 64 * 64
        magp = np.zeros((mag.shape[0], K), np.float32)
        magp[:, :nb] = mag
        melw = np.zeros((K, gen.NUM_MELS), np.float32)
        melw[:nb] = F.mel_filterbank(s["sampling_rate"], n_fft, gen.NUM_MELS, s["fmin"], s["fmax"]).astype(np.float32)
        en = np.sqrt(np.maximum(np.concatenate(pows), np.float32(1e-10)))
        m = gen.measures(chain(magp, melw), en, z[f"{name}_mel64"], z[f"{name}_energy64"], z[f"{name}_silent"])
        r = m / z[f"{name}_e32"]
        print(f"{name}: lin {m[0]:.3e} log {m[1]:.3e} en {m[2]:.3e} = {r[0]:.2f} / {r[1]:.2f} / {r[2]:.2f} x E32")


if __name__ == "__main__":
    main()
