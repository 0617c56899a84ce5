"""Pitch (csrc/pitch.hip): ``Pitch`` is the reference's ``feature_extract/dio.py:21-159``.  The reference extracts F0
with DIO + StoneMask through pyworld, which is absent from the build environment, so the raw track comes from an estimator of this
project's own: Boersma's 1993 autocorrelation method on the STFT's frames (``Stft.magnitude`` -> ``jatts_acf_from_mag``, the same exact-f32
MFMA contraction -> ``jatts_pitch_pick``; the definition is written out in csrc/pitch.hip), pinned on a float64 restatement
(tests/pitch_reference.py).  Parity with DIO / StoneMask is UNPINNED.  The steps after the raw track -- continuous F0, log, length
adjustment, token average -- ARE pinned on the real ``Dio.forward`` (``tests/golden/pitch_post_kat.npz``)."""
import collections
import math

import numpy as np
import torch

from .. import hip
from .common import PackedWaves, adjust_and_average, require_cuda
from .stft import Stft, check_stft_params

PITCH_VOICING_THRESHOLD, PITCH_SILENCE_THRESHOLD, PITCH_OCTAVE_COST = 0.45, 0.03, 0.01      # Boersma's defaults
PitchRange = collections.namedtuple("PitchRange", "lo hi sum_w2 stft acf")      # one (f0min, f0max): lags, sum w^2, front end of its window, ACF table


def pitch_geometry(sr, n_fft, f0min, f0max):
    """-> (lo, hi, W): the lag range lo = ceil(sr / f0max) .. hi = floor(sr / f0min) and the analysis window's length W = min(3 hi,
    n_fft - hi - 1) rounded down to even (W + hi < n_fft keeps the circular autocorrelation from wrapping).  ValueError when the
    window cannot hold two of the longest periods (W < 2 hi) or lo < 2."""
    if not 0 < f0min < f0max:
        raise ValueError(f"pitch: 0 < f0min < f0max expected (got {f0min}, {f0max})")
    lo, hi = int(math.ceil(sr / f0max)), int(math.floor(sr / f0min))
    w = min(3 * hi, n_fft - hi - 1) // 2 * 2
    if w < 2 * hi or lo < 2:
        raise ValueError(f"pitch: f0 range {f0min}-{f0max} Hz at {sr} Hz needs lags {lo}..{hi}, an fft_size of {n_fft} leaves a window of "
                         f"{max(w, 0)} samples (two periods of f0min and lo >= 2 are needed): raise f0min or fft_size")
    return lo, hi, w


def window_autocorrelation(window_padded, n_lags):
    """float64 (n_lags,): rw(tau) = sum_n w[n] w[n + tau]"""
    w = np.asarray(window_padded, dtype=np.float64)
    return np.array([np.dot(w[:w.size - t], w[t:]) for t in range(n_lags)], dtype=np.float64)


def acf_table(window_padded, n_fft, hi):
    """float32 (K, Lp), K = n_bins rounded up to 64, Lp = hi + 2 rounded up to 32 (what jatts_acf_from_mag takes): entry [k][tau] =
    c_k cos(2 pi k tau / n_fft) / n_fft * rw(0) / rw(tau), c_0 = c_{n_fft/2} = 1, else 2, for k < n_bins and tau <= hi + 1, zeros in the
    padding.  Angles are reduced in integers (k tau mod n_fft); the product is taken in float64 and rounded to f32 once."""
    n_bins = n_fft // 2 + 1
    k_rows, lp = hip.round_up(n_bins, 64), hip.round_up(hi + 2, 32)
    rw = window_autocorrelation(window_padded, hi + 2)
    if not (rw > 0.0).all():
        raise ValueError("pitch: the window's autocorrelation vanishes inside the lag range")
    kt = (np.arange(n_bins, dtype=np.int64)[:, None] * np.arange(hi + 2, dtype=np.int64)[None, :]) % n_fft
    c = np.full(n_bins, 2.0)
    c[0] = c[-1] = 1.0
    t = np.zeros((k_rows, lp), dtype=np.float32)
    t[:n_bins, :hi + 2] = (c[:, None] * np.cos((2.0 * np.pi / n_fft) * kt.astype(np.float64)) / n_fft * (rw[0] / rw)[None, :]).astype(np.float32)
    return t


class Pitch:
    """``Dio`` of the reference (dio.py:21-159) on the GPU, with the autocorrelation estimator above in place of pyworld: same
    constructor, ``forward(input, f0min, f0max, feat_length, durations)``: ndarray in, float32 ndarray out.  ``extract`` is the ragged
    entry over a ``PackedWaves``.  One ``PitchRange`` (the STFT front end of its window, the autocorrelation table) is kept per (f0min, f0max)."""

    def __init__(self, fs=22050, n_fft=1024, hop_length=256, use_token_averaged_f0=True, use_continuous_f0=True, use_log_f0=True,
                 reduction_factor=None, voicing_threshold=PITCH_VOICING_THRESHOLD, silence_threshold=PITCH_SILENCE_THRESHOLD,
                 octave_cost=PITCH_OCTAVE_COST, device="cuda"):
        if use_token_averaged_f0 and not (reduction_factor is not None and reduction_factor >= 1):
            raise ValueError(f"use_token_averaged_f0 needs reduction_factor >= 1 (got {reduction_factor})")      # dio.py:58-59
        check_stft_params(n_fft, hop_length)
        self.device = require_cuda(device)
        self.fs, self.n_fft, self.hop_length = fs, int(n_fft), int(hop_length)
        self.use_token_averaged_f0, self.use_continuous_f0, self.use_log_f0 = use_token_averaged_f0, use_continuous_f0, use_log_f0
        self.reduction_factor = reduction_factor
        self.voicing_threshold, self.silence_threshold, self.octave_cost = float(voicing_threshold), float(silence_threshold), float(octave_cost)
        self._ranges = {}

    def output_size(self):
        return 1

    def get_parameters(self):
        return dict(fs=self.fs, n_fft=self.n_fft, hop_length=self.hop_length, use_token_averaged_f0=self.use_token_averaged_f0,
                    use_continuous_f0=self.use_continuous_f0, use_log_f0=self.use_log_f0, reduction_factor=self.reduction_factor)

    def tables(self, f0min, f0max):
        """The ``PitchRange`` of a range, built once."""
        key = (float(f0min), float(f0max))
        if key not in self._ranges:
            lo, hi, w_len = pitch_geometry(self.fs, self.n_fft, f0min, f0max)
            stft = Stft(self.device, self.n_fft, self.hop_length, w_len)
            self._ranges[key] = PitchRange(lo, hi, float(np.dot(stft.window, stft.window)), stft,
                                           torch.from_numpy(acf_table(stft.window, self.n_fft, hi)).to(self.device))
        return self._ranges[key]

    @torch.no_grad()
    def raw(self, waves, f0min, f0max, peaks=None):
        """Steps 1-5 over a ``PackedWaves`` -> (RaggedBatch over frames, f0 f32 (rows,) with 0 for unvoiced frames, tau int32 (rows,)).
        ``peaks``: device f32 (n_seq,) max |x| per utterance (default: one ``jatts_wave_gain_peak`` launch with gain 1)."""
        if not isinstance(waves, PackedWaves):
            raise TypeError("Pitch.raw takes a PackedWaves")
        if not waves.lens:
            raise ValueError("no waveform")
        t = self.tables(f0min, f0max)
        if peaks is None:
            peak, stride = hip.wave_gain_peak(waves.cu, len(waves.lens), waves.x, 1.0), 2      # (x * 1.0: the samples keep their bits)
        else:
            peak, stride = peaks.to(torch.float32).contiguous(), 1
        rb, mag, _ = t.stft.magnitude(waves)
        r = hip.acf_from_mag(rb, mag, t.acf)
        f0, tau = hip.pitch_pick(rb, r, peak, stride, t.lo, t.hi, self.fs, f0min, t.sum_w2, self.voicing_threshold, self.silence_threshold,
                                 self.octave_cost)
        return rb, f0, tau

    @torch.no_grad()
    def post(self, rb, f0, feat_lengths=None, durations=None):
        """Step 6 on a raw track (dio.py:110-159) -> list of per-utterance f32 device tensors."""
        p = hip.f0_continuous_log(rb, f0, self.use_continuous_f0, self.use_log_f0)
        if self.use_token_averaged_f0 and durations is None:
            raise ValueError("use_token_averaged_f0 needs durations: one sequence per utterance")
        return adjust_and_average(rb, p, feat_lengths, durations if self.use_token_averaged_f0 else None, self.reduction_factor)

    def extract(self, waves, f0min, f0max, feat_lengths=None, durations=None, peaks=None):
        """The ragged entry: a ``PackedWaves`` of utterances that share one f0 range -> list of per-utterance f32 device tensors."""
        rb, f0, _ = self.raw(waves, f0min, f0max, peaks)
        return self.post(rb, f0, feat_lengths, durations)

    def forward(self, input, f0min=80, f0max=400, feat_length=None, durations=None):
        pw = PackedWaves.from_list([np.asarray(input)], self.device)
        out = self.extract(pw, f0min, f0max, None if feat_length is None else [int(feat_length)],
                           [durations] if self.use_token_averaged_f0 else None)
        return out[0].cpu().numpy()
