"""Shared by tests/test_pitch_cpu.py and tests/test_pitch_gpu.py: a float64 restatement of the autocorrelation F0 estimator's definition
(DESIGN §7 f.8, steps 1-5), the reference's post-processing restated (step 6; pinned separately on tests/golden/pitch_post_kat.npz), and the
test signals.

The restatement is np.fft based and never touches the kernels' tables (features.dft_table / features.acf_table): frames are cut from
np.pad(mode="reflect"), the window is built here, the autocorrelation is irfft(|rfft|^2) and the window's own is taken the same way.

`analyse` also says which frames are FRAGILE: those whose decision, in float64 alone, hangs on less than 1e-3 -- the winner's score leads the
runner-up by < 1e-3, the winner's peak is within 1e-3 of the voicing threshold, or the level ratio is within 1e-3 of the silence threshold.
A float32 computation may legitimately decide those the other way."""
import math

import numpy as np

FRAGILE = 1e-3


def geometry(sr, n_fft, f0min, f0max):
    lo, hi = int(math.ceil(sr / f0max)), int(math.floor(sr / f0min))
    w = min(3 * hi, n_fft - hi - 1)
    w -= w % 2
    return lo, hi, w


def hann_padded(w_len, n_fft):
    n = np.arange(w_len, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / w_len)          # periodic Hann
    out = np.zeros(n_fft)
    left = (n_fft - w_len) // 2
    out[left:left + w_len] = w
    return out


def frames_of(x, n_fft, hop):
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    t = 1 + x.size // hop
    idx = np.arange(t)[:, None] * hop + np.arange(n_fft)[None, :]
    return xp[idx]


def analyse(x, sr, n_fft, hop, f0min, f0max, voicing=0.45, silence=0.03, octave=0.01):
    """-> dict of per-frame arrays: f0 (0 = unvoiced), tau (0 = no candidate), off, peak, ratio, voiced, cand, margin, fragile; and the
    scalars lo, hi, W."""
    lo, hi, w_len = geometry(sr, n_fft, f0min, f0max)
    assert w_len >= 2 * hi and lo >= 2
    w = hann_padded(w_len, n_fft)
    fr = frames_of(x, n_fft, hop) * w[None, :]
    r = np.fft.irfft(np.abs(np.fft.rfft(fr, axis=1)) ** 2, n=n_fft, axis=1)[:, :hi + 2]
    rw = np.fft.irfft(np.abs(np.fft.rfft(w)) ** 2, n=n_fft)[:hi + 2]
    rho = r / np.maximum(r[:, :1], 1e-30) * (rw[0] / rw)[None, :]
    a, b, c = rho[:, lo - 1:hi], rho[:, lo:hi + 1], rho[:, lo + 1:hi + 2]
    cand = (b >= a) & (b > c)
    den = a - 2.0 * b + c
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.where(den < 0.0, np.clip(0.5 * (a - c) / den, -0.5, 0.5), 0.0)
    peak = b - 0.25 * (a - c) * off
    taus = np.arange(lo, hi + 1, dtype=np.float64)[None, :]
    score = np.where(cand, peak - octave * np.log2((taus + off) * f0min / sr), -np.inf)
    win = np.argmax(score, axis=1)                            # the first maximum: equal scores go to the smallest tau
    rows = np.arange(score.shape[0])
    has = cand.any(axis=1)
    best = score[rows, win]
    rest = score.copy()
    rest[rows, win] = -np.inf
    margin = np.where(has, best - rest.max(axis=1), np.inf)
    w_off, w_peak = off[rows, win], peak[rows, win]
    x_max = float(np.abs(np.asarray(x, dtype=np.float64)).max())
    level = np.sqrt(r[:, 0] / np.dot(w, w))
    ratio = level / x_max if x_max > 0.0 else np.zeros_like(level)
    voiced = has & (w_peak >= voicing) & (level >= silence * x_max)
    tau = np.where(has, win + lo, 0)
    with np.errstate(divide="ignore"):
        f0 = np.where(voiced, sr / (tau + w_off), 0.0)
    fragile = (has & (margin < FRAGILE)) | (has & (np.abs(w_peak - voicing) < FRAGILE)) | (np.abs(ratio - silence) < FRAGILE)
    return dict(f0=f0, tau=tau, off=np.where(has, w_off, 0.0), peak=np.where(has, w_peak, 0.0), ratio=ratio, voiced=voiced, cand=has,
                margin=margin, fragile=fragile, lo=lo, hi=hi, W=w_len)


# ---- step 6, restated from jatts/modules/feature_extract/dio.py:110-159 (float64)
def continuous_f0(f0):
    f0 = np.array(f0, dtype=np.float64)
    nz = np.flatnonzero(f0)
    if nz.size == 0:
        return f0
    f0[:nz[0]] = f0[nz[0]]
    f0[nz[-1]:] = f0[nz[-1]]
    nz = np.flatnonzero(f0)
    return np.interp(np.arange(f0.size), nz, f0[nz])


def post(f0, feat_length=None, durations=None, continuous=True, log=True):
    p = continuous_f0(f0) if continuous else np.array(f0, dtype=np.float64)
    if log:
        p[p != 0] = np.log(p[p != 0])
    if feat_length is not None:
        p = np.pad(p, (0, feat_length - p.size)) if feat_length > p.size else p[:feat_length]
    if durations is None:
        return p
    ends = np.cumsum(durations)
    out = []
    for s, e in zip(np.concatenate([[0], ends[:-1]]), ends):
        seg = p[s:e]
        seg = seg[seg > 0.0]
        out.append(seg.mean() if seg.size else 0.0)
    return np.array(out, dtype=np.float64)


# ---- signals
def make_signal(sr, f_start, f_end, seconds, seed, gate=0.1):
    """8 harmonics (amplitudes 0.8^h, random phases) on a linear f0 sweep, silent gates of `gate` seconds at the start, in the middle and at
    the end, additive noise of 1e-3, a peak of 0.5 -> (x float32, f_true per sample, voiced per sample)."""
    g = np.random.default_rng(seed)
    n = int(round(seconds * sr))
    f = np.linspace(f_start, f_end, n)
    phase = 2.0 * np.pi * np.cumsum(f) / sr
    x = np.zeros(n)
    for h in range(1, 9):
        x += 0.8 ** h * np.sin(h * phase + g.uniform(0.0, 2.0 * np.pi))
    x *= 0.5 / np.abs(x).max()
    ng = int(round(gate * sr))
    on = np.ones(n, dtype=bool)
    on[:ng] = False
    on[n // 2 - ng // 2:n // 2 - ng // 2 + ng] = False
    on[n - ng:] = False
    x = np.where(on, x, 0.0) + 1e-3 * g.standard_normal(n)
    return x.astype(np.float32), f, on


def frame_truth(f_true, on, hop, w_len):
    """Per frame: the sweep's frequency at the frame's centre, whether the whole analysis window lies in voiced signal, whether it lies
    wholly inside a silent gate (windows that reach past either end of the signal are neither)."""
    n = on.size
    t = 1 + n // hop
    centre = np.arange(t) * hop
    a, b = centre - w_len // 2, centre + w_len // 2
    inside = (a >= 0) & (b <= n)
    csum = np.concatenate([[0], np.cumsum(on)])
    count = csum[np.clip(b, 0, n)] - csum[np.clip(a, 0, n)]
    full = inside & (count == w_len)
    silent = inside & (count == 0)
    return f_true[np.clip(centre, 0, n - 1)], full, silent
