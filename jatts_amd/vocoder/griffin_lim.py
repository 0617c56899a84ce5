"""Griffin-Lim on HIP: the waveform of a (log-mel) spectrogram without a trained vocoder -- what the reference means by
``Spectrogram2Waveform(..., griffin_lim_iters=64)`` (``tts_decode.py:190-200``, ``tts_train.py:316-325``) wherever a config has no
``vocoder:`` entry.  The reference's own module does not exist (its import is commented out) and librosa is absent from the build
environment, so the arithmetic is a definition of THIS project's, pinned on a float64 restatement (``tests/griffinlim_reference.py``);
parity with ``librosa.griffinlim`` and ESPnet's ``logmel2linear`` is UNPINNED.

    X_0 = S * P0;  C_-1 = 0;  beta = momentum / (1 + momentum)
    n_iter times:  x = ISTFT(X);  C = STFT(x);  A = C - beta * C_prev;  X = S * A / (|A| + 2^-126)
    y = ISTFT(X)

STFT: centred frames, zero padding, the padded periodic Hann window (``torch.stft(center=True, pad_mode="constant")``); ISTFT: the windowed
overlap-add divided by the summed squared windows (``torch.istft(center=True, length=(T - 1) * hop)``).  Both are exact-f32 MFMA contractions
(``csrc/griffinlim.hip``); torch / numpy prepare constants (tables, the initial phases), never the arithmetic.  Mel to linear:
``max(1e-10, pinv(B) @ base ** (c * scale + mean))`` with B the Slaney basis of ``features.stft.mel_filterbank``."""
import logging
import math
import time

import numpy as np
import torch

from .. import _abi, hip
from .._abi import F32
from ..features.common import require_cuda
from ..features.stft import check_stft_params, dft_table, mel_filterbank, padded_window
from .vocoder import read_stats

MAX_OVERLAP = 64          # GL_MAX_J of csrc/griffinlim.hip: frames that overlap one sample
NOLA_FLOOR = 1e-11        # torch.istft's: the smallest summed squared window it divides by
CONFIG_KEYS = ("fft_size", "hop_size", "sampling_rate", "num_mels", "fmin", "fmax")      # what a config must carry for the fallback


# ---- constants (float64 on the host)
def overlap(n_fft, hop):
    """J: the frames that can overlap one sample"""
    return -(-n_fft // hop)


def istft_table(window_padded, n_fft, hop, dtype=np.float32):
    """float32 (J * 2 * nbp, hopp), hopp = hop rounded up to 32: the synthesis table of ``jatts_gl_istft``.  Row i * 2 nbp + k, column r, with
    q = (J - 1 - i) * hop + r: c_k cos(2 pi k q / n_fft) w[q] / n_fft for the real plane (k < n_bins), -c_k sin(..) w[q] / n_fft for the
    imaginary plane (nbp + k); 0 where q >= n_fft and in the padding; c_k = 1 at DC and Nyquist, 2 elsewhere.  Angles are reduced in integers,
    the products taken in float64 and rounded to f32 once (``dtype=np.float64``: not rounded, for the tests)."""
    n_bins = n_fft // 2 + 1
    nbp, hopp, J = hip.round_up(n_bins, 32), hip.round_up(hop, 32), overlap(n_fft, hop)
    w = np.zeros(J * hop, dtype=np.float64)
    w[:n_fft] = np.asarray(window_padded, dtype=np.float64)
    ck = np.full(n_bins, 2.0)
    ck[0] = ck[-1] = 1.0
    k = np.arange(n_bins, dtype=np.int64)[:, None]
    t = np.zeros((J, 2 * nbp, hopp), dtype=dtype)
    for i in range(J):
        q = (J - 1 - i) * hop + np.arange(hop, dtype=np.int64)[None, :]
        ang = (2.0 * np.pi / n_fft) * ((k * q) % n_fft).astype(np.float64)
        g = ck[:, None] * w[q] / n_fft                     # (n_bins, hop); zero where q >= n_fft
        t[i, :n_bins, :hop] = (g * np.cos(ang)).astype(dtype)
        t[i, nbp:nbp + n_bins, :hop] = (-g * np.sin(ang)).astype(dtype)
    return t.reshape(J * 2 * nbp, hopp)


def envelope_sums(window_padded, n_fft, hop):
    """float64 (J, J, hop): E[a][b][r] = sum_{a <= j <= b} w^2[j * hop + r] (0 for a > b) -- the summed squared windows at position
    p = m * hop + r of an utterance of T frames, with (a, b) = (max(0, m - T + 1), min(J - 1, m)): the frames m - j that exist."""
    J = overlap(n_fft, hop)
    w2 = np.zeros(J * hop, dtype=np.float64)
    w2[:n_fft] = np.asarray(window_padded, dtype=np.float64) ** 2
    w2 = w2.reshape(J, hop)
    e = np.zeros((J, J, hop), dtype=np.float64)
    for a in range(J):
        s = np.zeros(hop, dtype=np.float64)
        for b in range(a, J):
            s = s + w2[b]
            e[a, b] = s
    return e


def istft_envelope(window_padded, n_fft, hop):
    """float32 (J, J, hopp): 1 / envelope_sums rounded once; 0 where the sum is below the NOLA floor (never inside an output range of a
    geometry ``check_nola`` accepts) and in the padding columns."""
    e = envelope_sums(window_padded, n_fft, hop)
    J, hopp = e.shape[0], hip.round_up(hop, 32)
    out = np.zeros((J, J, hopp), dtype=np.float32)
    ok = e >= NOLA_FLOOR
    out[:, :, :hop][ok] = (1.0 / e[ok]).astype(np.float32)
    return out


def envelope_index(T, n_fft, hop):
    """(a, b, r) int64 arrays over the output samples n < (T - 1) * hop of an utterance of T frames: its envelope is E[a, b, r]."""
    J = overlap(n_fft, hop)
    p = np.arange((T - 1) * hop, dtype=np.int64) + n_fft // 2
    m = p // hop
    return np.maximum(0, m - T + 1), np.minimum(J - 1, m), p - m * hop


def check_nola(env, T, n_fft, hop):
    """ValueError where the summed squared windows fall below torch's floor inside the output range of an utterance of T frames."""
    if T < 2:
        return
    a, b, r = envelope_index(T, n_fft, hop)
    low = float(env[a, b, r].min())
    if low < NOLA_FLOOR:
        raise ValueError(f"fft_size {n_fft}, hop_size {hop}: the summed squared windows fall to {low:.3e} inside an utterance of {T} frames "
                         f"(below {NOLA_FLOOR}): the inverse STFT is undefined there (is hop_size larger than win_length?)")


_TABLES = None


def tables_cache():
    """The registered DeviceCache of the tables, (n_fft, hop, win_length, window) -> (DFT, ISTFT, reciprocal envelope).  It is made at the first
    use, not at import: a process that never runs Griffin-Lim registers nothing (tests/test_device_cache_cpu.py pins the caches an import
    registers)."""
    global _TABLES
    if _TABLES is None:
        _TABLES = hip.DeviceCache("griffin_lim tables", max_entries=4, register=True)
    return _TABLES


class GriffinLim:
    """The loop above for one (n_fft, hop, window).  ``gl(rb_frames, S, init=None, seed=0)`` -> (lens, y): the per-utterance sample counts
    (T_b - 1) * hop and the packed f32 waveform, utterances back to back.  ``S``: f32 device (rows, >= n_bins) linear magnitudes, >= 0.
    ``init``: unit-modulus complex64 (rows, n_bins); None: 2 pi * torch.rand from a device generator seeded with ``seed``, turned into P0
    with torch once per call (input data, not the arithmetic) -- two calls with the same seed give identical bits.
    ValueError: a geometry outside the kernels' limits, ``momentum`` outside [0, 1), ``n_iter`` < 0, and a (hop, window) whose summed
    squared windows fall below 1e-11 inside an output range (torch's NOLA rule; ``hop > win_length`` is one)."""

    def __init__(self, device, n_fft, hop, win_length=None, window="hann", n_iter=64, momentum=0.99):
        check_stft_params(n_fft, hop)
        self.n_fft, self.hop, self.n_iter, self.momentum = int(n_fft), int(hop), int(n_iter), float(momentum)
        if self.n_iter < 0 or self.n_iter != n_iter:
            raise ValueError(f"n_iter {n_iter} must be a non-negative integer")
        if not 0.0 <= self.momentum < 1.0:
            raise ValueError(f"momentum {momentum} must lie in [0, 1)")
        self.J = overlap(self.n_fft, self.hop)
        if self.J > MAX_OVERLAP:
            raise ValueError(f"hop_size {hop} is below fft_size / {MAX_OVERLAP} (more than {MAX_OVERLAP} overlapping frames)")
        self.beta = self.momentum / (1.0 + self.momentum)
        self.window = padded_window(window, win_length, self.n_fft)
        self.n_bins = self.n_fft // 2 + 1
        self.nbp = hip.round_up(self.n_bins, 32)
        self._env = envelope_sums(self.window, self.n_fft, self.hop)
        self._nola_ok = {2 * self.J + 2}          # frame counts checked; from 2 J + 2 on, head, interior and tail are those of 2 J + 2
        check_nola(self._env, 2 * self.J + 2, self.n_fft, self.hop)
        self._key = (self.n_fft, self.hop, None if win_length is None else int(win_length), window)
        self.device = require_cuda(device, "jatts_amd.vocoder.GriffinLim")
        _abi.load()

    def tables(self):
        """-> (DFT table, ISTFT table, reciprocal envelope) on the device, from the registered cache"""
        def build():
            return tuple(torch.from_numpy(a).to(self.device) for a in (dft_table(self.window, self.n_fft),
                                                                       istft_table(self.window, self.n_fft, self.hop),
                                                                       istft_envelope(self.window, self.n_fft, self.hop)))
        return tables_cache().get(self._key, self.device, build)

    def _check_frames(self, rb):
        for T in set(rb.lens):
            if T < 1:
                raise ValueError("GriffinLim: every utterance needs at least one frame")
            if T < 2 * self.J + 2 and T not in self._nola_ok:
                check_nola(self._env, T, self.n_fft, self.hop)
                self._nola_ok.add(T)

    def initial_phases(self, rows, seed=0):
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        ph = torch.rand(rows, self.n_bins, generator=g, device=self.device, dtype=torch.float32) * (2.0 * math.pi)
        return torch.polar(torch.ones_like(ph), ph)

    @torch.no_grad()
    def run(self, rb, S, init=None, seed=0, y=None, packed=True, n_iter=None):
        """The loop into ``y``: ``packed``, the utterances back to back ((rows - n_seq) * hop floats); else the frame layout, utterance b at
        cu_rows[b] * hop (rows * hop floats, the last hop of each not written).  Scratch (X, C_prev, x) is allocated once per call."""
        self._check_frames(rb)
        if not isinstance(S, torch.Tensor) or not S.is_cuda or S.dtype != torch.float32 or S.dim() != 2 or not S.is_contiguous() \
                or S.shape[0] != rb.total or S.shape[1] < self.n_bins:
            raise ValueError("GriffinLim: S must be a contiguous float32 device matrix (rows, >= n_bins)")
        n_iter = self.n_iter if n_iter is None else int(n_iter)
        dft, tab, renv = self.tables()
        rows = rb.total
        p0 = self.initial_phases(rows, seed) if init is None else init.to(torch.complex64).contiguous()
        X = torch.empty(max(rows, 1), 2 * self.nbp, dtype=torch.float32, device=S.device)
        if y is None:
            y = torch.empty(max((rows - (rb.n_seq if packed else 0)) * self.hop, 1), dtype=torch.float32, device=S.device)
        if rows == 0:
            return y
        hip.gl_init(S, p0, self.n_fft, X)
        if n_iter:
            c_prev = torch.zeros_like(X)
            x = torch.empty(rows * self.hop, dtype=torch.float32, device=S.device)
            for _ in range(n_iter):
                hip.gl_istft(rb, X, tab, renv, self.n_fft, self.hop, x, False)
                hip.gl_stft_project(rb, x, dft, self.n_fft, self.hop, S, self.beta, c_prev, X)
        return hip.gl_istft(rb, X, tab, renv, self.n_fft, self.hop, y, packed)

    def __call__(self, rb_frames, S, init=None, seed=0):
        lens = [(T - 1) * self.hop for T in rb_frames.lens]
        return lens, self.run(rb_frames, S, init, seed)[:sum(lens)]


def _log_code(log_base):
    try:
        return {None: 0, 2.0: 2, 10.0: 10}[None if log_base is None else float(log_base)]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{log_base} is not supported.") from None


def mel_pinv(fs, n_fft, n_mels, fmin=None, fmax=None):
    """float32 (n_bins, n_mels): numpy.linalg.pinv of the (n_mels, n_bins) Slaney basis in float64, rounded once."""
    return np.linalg.pinv(mel_filterbank(fs, n_fft, n_mels, fmin, fmax).T).astype(np.float32)


class Spectrogram2Waveform:
    """The reference's call (``tts_decode.py:191-200``: stats, n_fft, n_shift, fs, n_mels, fmin, fmax, griffin_lim_iters) plus the three
    analysis parameters it forgets to pass (win_length, window, log_base), with what the two call sites use of ``Vocoder``:
    ``decode(c) -> (y, fs)`` with y of (T - 1) * hop samples, ``decode_batch(rb, mel)``, ``config["sampling_rate"]``, ``hop`` and
    ``set_precision``.  ``stats``: a {"mean", "scale"} dict, an .npz path, or .h5 where h5py imports (``vocoder.read_stats``).
    Normalised log-mel features c -> ``lin = max(1e-10, pinv(B) @ base ** (c * scale + mean))`` -> ``GriffinLim``.  The pseudo-inverse
    projection is a k = 1 ``PackedConv`` in exact f32, whatever the precision of the model in front of it."""

    def __init__(self, stats, n_fft, n_shift, fs, n_mels, fmin, fmax, griffin_lim_iters=64, win_length=None, window="hann", log_base=10.0,
                 device="cuda", momentum=0.99):
        self.log_code = _log_code(log_base)
        self.gl = GriffinLim(device, n_fft, n_shift, win_length, window, griffin_lim_iters, momentum)
        self.device, self.hop, self.n_mels = self.gl.device, self.gl.hop, int(n_mels)
        self.config = {"sampling_rate": int(fs), "griffin_lim_iters": self.gl.n_iter}
        mean, scale = read_stats(stats)
        if mean.shape != (self.n_mels,) or scale.shape != (self.n_mels,):
            raise ValueError(f"stats of {mean.shape[0]} channels for num_mels = {self.n_mels}")
        self.mean, self.scale = torch.from_numpy(mean).to(self.device), torch.from_numpy(scale).to(self.device)
        self.ld_mel = hip.round_up(self.n_mels, 64)
        with hip.operands(None):     # exact f32 always
            self.proj = hip.PackedConv(torch.from_numpy(mel_pinv(fs, self.gl.n_fft, self.n_mels, fmin, fmax)), None, F32, self.device)

    @classmethod
    def from_config(cls, config, stats, device):
        """From a recipe config's top-level keys; a missing one is a ValueError naming it."""
        for k in CONFIG_KEYS:
            if k not in config:
                raise ValueError(f"the Griffin-Lim fallback (no vocoder in the config) needs '{k}' in the config")
        return cls(stats, config["fft_size"], config["hop_size"], config["sampling_rate"], config["num_mels"], config["fmin"], config["fmax"],
                   griffin_lim_iters=config.get("griffin_lim_iters", 64), win_length=config.get("win_length"), window=config.get("window", "hann"),
                   log_base=config.get("log_base", 10.0), device=device)

    def set_precision(self, precision):
        """Accepted for the interface and returns self: the arithmetic is exact f32 in every precision."""
        return self

    @torch.no_grad()
    def linear(self, rb, c):
        """Normalised log-mel c (rows, >= n_mels) -> linear magnitudes f32 (rows, nbp), padding columns zero"""
        c = c.to(self.device).float().contiguous()
        mel = hip.gl_exp(c, self.n_mels, self.scale, self.mean, self.log_code, self.ld_mel)
        return hip.gl_floor(self.proj(rb, mel), self.gl.n_bins, 1e-10, self.gl.nbp)

    @torch.no_grad()
    def decode_batch(self, rb, mel, init=None, seed=0):
        """Packed ragged batch: mel f32 (rows, n_mels) -> packed waveform f32 (rows * hop,) in ``Vocoder.decode_batch``'s layout: utterance b
        sits at cu_rows[b] * hop.  It has (T_b - 1) * hop samples, so its last hop samples are zero: a 1-hop silent tail."""
        y = torch.zeros(max(rb.total * self.hop, 1), dtype=torch.float32, device=self.device)
        return self.gl.run(rb, self.linear(rb, mel), init, seed, y=y, packed=False)[:rb.total * self.hop]

    @torch.no_grad()
    def decode(self, c):
        start = time.time()
        rb = hip.RaggedBatch([c.shape[0]], self.device)
        y = self.decode_batch(rb, c)[:(c.shape[0] - 1) * self.hop]
        rtf = (time.time() - start) / max(len(y) / self.config["sampling_rate"], 1e-9)
        logging.info(f"Finished waveform generation by Griffin-Lim, {self.gl.n_iter} iterations. (RTF = {rtf:.03f}).")
        return y, self.config["sampling_rate"]
