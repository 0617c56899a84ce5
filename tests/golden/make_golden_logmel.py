"""Writes tests/golden/logmel_kat.npz: known-answer data for jatts_amd.features (tests/test_features_cpu.py, tests/test_features_gpu.py).

Run on a CPU host (python tests/golden/make_golden_logmel.py); never run by the test suite.

librosa is not installed where this project is built, so the reference's own feature extraction cannot produce the answers and parity
with librosa itself stays UNPINNED.  The answers come from two independent implementations instead:
  * torch.stft in float64 (center=True, pad_mode="reflect", periodic Hann window, torch's own centring of a short window);
  * transformers.audio_utils.mel_filter_bank(norm="slaney", mel_scale="slaney") in float64.
Nothing here imports jatts_amd.

Per setting the file also holds the float32-FFT yardstick E32: the same three error measures the GPU test applies to the kernel,
taken for the float32 restatement (torch.stft of float32 audio in complex64, float32 mel matrix, float32 log) -- the arithmetic
class of the reference (librosa's STFT of float32 audio is complex64).  The kernel may be 8 x E32 per measure.
"""
import os

import numpy as np
import torch
from transformers.audio_utils import mel_filter_bank

HERE = os.path.dirname(os.path.abspath(__file__))
NUM_MELS, EPS = 80, 1e-10
SETTINGS = {
    "a": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=2048, fmin=80, fmax=7600),
    "b": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=1200, fmin=80, fmax=7600),
    "c": dict(sampling_rate=22050, fft_size=1024, hop_size=256, win_length=None, fmin=None, fmax=None),
}


def lengths(n_fft, hop):
    return [n_fft // 2 + 1, 7 * hop, 20000, 6000 + n_fft]


def signal(n, sr, rng):
    """Harmonic tone with a moving f0 under a squared-sine envelope, plus noise at 1e-4: strong and weak bins in every frame."""
    t = np.arange(n) / sr
    f0 = 140.0 + 60.0 * np.sin(2 * np.pi * 1.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(a * np.sin(h * ph + rng.uniform(0, 6.28)) for h, a in ((1, 0.5), (2, 0.25), (3, 0.12), (5, 0.06), (9, 0.03)))
    env = np.sin(2 * np.pi * 2.3 * t + rng.uniform(0, 6.28)) ** 2
    return (0.6 * env * x + 1e-4 * rng.standard_normal(n)).astype(np.float32)


def stft_mag(x, n_fft, hop, win_length, dtype):
    win_length = n_fft if win_length is None else win_length
    # the window in float64, rounded once (scipy's / librosa's order): a float32 0.5 - 0.5 cos() cancels near the window's ends
    w = torch.hann_window(win_length, periodic=True, dtype=torch.float64).to(dtype)
    s = torch.stft(torch.from_numpy(x).to(dtype), n_fft, hop_length=hop, win_length=win_length, window=w, center=True,
                   pad_mode="reflect", return_complex=True)
    return s.abs().T.contiguous()                                   # (frames, bins)


def measures(mel, en, mel64, en64, silent, log=np.log10):
    """lin: max over non-silent frames of max_m |mel - mel64| / max_m mel64[t]; log: max |log mel - log mel64| over bins with
    mel64 >= 1e-3 x their frame's maximum; en: max relative energy error over non-silent frames."""
    live = ~silent
    top = mel64[live].max(axis=1, keepdims=True)
    lin = float((np.abs(mel[live].astype(np.float64) - mel64[live]) / top).max())
    strong = mel64[live] >= 1e-3 * top
    lg = float(np.abs(log(np.maximum(EPS, mel[live].astype(np.float64))) - log(np.maximum(EPS, mel64[live])))[strong].max())
    e = float((np.abs(en[live].astype(np.float64) - en64[live]) / en64[live]).max())
    return np.array([lin, lg, e])


def main():
    out = {}
    for name, s in SETTINGS.items():
        rng = np.random.default_rng({"a": 11, "b": 12, "c": 13}[name])
        sr, n_fft, hop = s["sampling_rate"], s["fft_size"], s["hop_size"]
        fmin = 0.0 if s["fmin"] is None else float(s["fmin"])
        fmax = sr / 2.0 if s["fmax"] is None else float(s["fmax"])
        melmat = mel_filter_bank(n_fft // 2 + 1, NUM_MELS, fmin, fmax, sr, norm="slaney", mel_scale="slaney").astype(np.float64)
        waves = [signal(n, sr, rng) for n in lengths(n_fft, hop)]
        z0 = (len(waves[3]) - (n_fft + 3 * hop)) // 2
        waves[3][z0:z0 + n_fft + 3 * hop] = 0.0                      # fully silent frames
        mag64 = np.concatenate([stft_mag(w, n_fft, hop, s["win_length"], torch.float64).numpy() for w in waves])
        mag32 = np.concatenate([stft_mag(w, n_fft, hop, s["win_length"], torch.float32).numpy() for w in waves])
        mel64 = mag64 @ melmat
        en64 = np.sqrt(np.maximum((mag64 ** 2).sum(axis=1), 1e-10))
        silent = mag64.max(axis=1) == 0.0
        assert silent.sum() >= 2 and not silent[:-20].any()
        mel32 = mag32 @ melmat.astype(np.float32)
        en32 = np.sqrt(np.maximum((mag32 ** 2).sum(axis=1), np.float32(1e-10)))
        assert mel32.dtype == np.float32 and en32.dtype == np.float32
        out[f"{name}_melmat"] = melmat
        out[f"{name}_wave"] = np.concatenate(waves)
        out[f"{name}_lens"] = np.array([len(w) for w in waves], dtype=np.int64)
        out[f"{name}_frames"] = np.array([1 + len(w) // hop for w in waves], dtype=np.int64)
        out[f"{name}_logmel64"] = np.log10(np.maximum(EPS, mel64))
        out[f"{name}_mel64"] = mel64
        out[f"{name}_energy64"] = en64
        out[f"{name}_silent"] = silent
        out[f"{name}_e32"] = measures(mel32, en32, mel64, en64, silent)
        print(name, "frames", out[f"{name}_frames"], "silent", int(silent.sum()), "E32 lin/log/en", out[f"{name}_e32"])
    path = os.path.join(HERE, "logmel_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
