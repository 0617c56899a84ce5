"""Log-mel filterbank and energy: the reference's ``jatts/modules/feature_extract/mel.py:11-73`` (``logmelfilterbank``) and
``feature_extract/energy.py:69-122`` (``Energy.forward``), which run librosa on one CPU thread.  The magnitude STFT is one exact-f32
MFMA contraction over raw samples (``jatts_stft_mag``: reflect padding while the operand is staged, the periodic Hann window folded
into the DFT table) behind one front end object, ``Stft``, which the pitch extractor uses too; the mel projection is a ``jatts_conv1d``
launch, the rest row-wise kernels.  torch / numpy prepare constants (window, mel matrix, DFT table), never the arithmetic.
librosa itself is absent from the build environment, so parity with it is NOT pinned; the tests pin this module on ``torch.stft`` in
float64 and on ``transformers.audio_utils.mel_filter_bank(norm="slaney", mel_scale="slaney")``."""
import functools
import math

import numpy as np
import torch

from .. import _abi, hip
from .._abi import F32
from .common import PackedWaves, adjust_and_average, require_cuda

# ---- constants (float64 on the host)
def _hz_to_mel(f):
    """Slaney's auditory-toolbox scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic (27 steps per factor 6.4) above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (math.log(6.4) / 27.0), lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), m * (200.0 / 3.0))


def mel_filterbank(sr, n_fft, n_mels, fmin=None, fmax=None):
    """float64 (n_fft // 2 + 1, n_mels): triangular filters on the Slaney mel scale, each scaled by 2 / bandwidth -- what
    ``librosa.filters.mel`` gives with its defaults (htk=False, norm="slaney"; mel.py:55-63), restated from the published formula."""
    fmin = 0.0 if fmin is None else float(fmin)
    fmax = sr / 2.0 if fmax is None else float(fmax)
    n_bins = n_fft // 2 + 1
    freqs = np.linspace(0.0, sr / 2.0, n_bins)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[None, :] - freqs[:, None]                         # (n_bins, n_mels + 2)
    rising, falling = -ramps[:, :-2] / width[:-1], ramps[:, 2:] / width[1:]
    return np.maximum(0.0, np.minimum(rising, falling)) * (2.0 / (edges[2:] - edges[:-2]))[None, :]


def padded_window(window, win_length, n_fft):
    """float64 (n_fft,): the periodic Hann window of ``win_length`` (default n_fft) centred in zeros, as librosa.stft / torch.stft pad it."""
    if window != "hann":
        raise ValueError(f"window {window!r} is not supported (only 'hann')")
    win_length = n_fft if win_length is None else int(win_length)
    if not 1 <= win_length <= n_fft:
        raise ValueError(f"win_length {win_length} must lie in [1, fft_size = {n_fft}]")
    w = 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, win_length + 1)[:-1])
    out = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    out[left:left + win_length] = w
    return out


def dft_table(window_padded, n_fft):
    """float32 (n_fft, 2 * nbp), nbp = n_bins rounded up to 32 (the kernel's bin tile): column k = w[n] cos(2 pi n k / n_fft), column
    nbp + k = -w[n] sin(2 pi n k / n_fft), zeros in the padding columns.  Angles are reduced in integers (n k mod n_fft), the product
    with the window is taken in float64 and rounded to f32 once."""
    n_bins = n_fft // 2 + 1
    nbp = hip.round_up(n_bins, 32)
    nk = (np.arange(n_fft, dtype=np.int64)[:, None] * np.arange(n_bins, dtype=np.int64)[None, :]) % n_fft
    ang = (2.0 * np.pi / n_fft) * nk.astype(np.float64)
    w = np.asarray(window_padded, dtype=np.float64)[:, None]
    t = np.zeros((n_fft, 2 * nbp), dtype=np.float32)
    t[:, :n_bins] = (w * np.cos(ang)).astype(np.float32)
    t[:, nbp:nbp + n_bins] = (-w * np.sin(ang)).astype(np.float32)
    return t


# ---- framing geometry (what the kernel applies while it stages its operand)
def frame_count(n_samples, n_fft, hop):
    """Frames of an utterance under center=True: 1 + n_samples // hop.  Raises for an utterance reflect padding cannot serve."""
    if n_samples <= n_fft // 2:
        raise ValueError(f"an utterance of {n_samples} samples is too short to be reflect-padded by {n_fft // 2} (fft_size {n_fft})")
    return 1 + n_samples // hop


def reflect_index(p, n_samples):
    """numpy.pad(mode="reflect") as an index map (no edge repeat): -i -> i, n_samples - 1 + i -> n_samples - 1 - i."""
    p = np.abs(np.asarray(p, dtype=np.int64))
    return np.where(p >= n_samples, 2 * (n_samples - 1) - p, p)


def frame_indices(n_samples, n_fft, hop):
    """int64 (frames, n_fft): the sample each element of each frame reads."""
    t = np.arange(frame_count(n_samples, n_fft, hop), dtype=np.int64)[:, None]
    return reflect_index(t * hop + np.arange(n_fft, dtype=np.int64)[None, :] - n_fft // 2, n_samples)


def check_stft_params(fft_size, hop_size):
    if fft_size % 64 or not 64 <= fft_size <= 2048:
        raise ValueError(f"fft_size {fft_size} must be a multiple of 64, at most 2048")
    if not 1 <= hop_size <= fft_size:
        raise ValueError(f"hop_size {hop_size} must lie in [1, fft_size]")


class Stft:
    """The STFT front end of one (n_fft, hop, window), the one caller of ``hip.stft_mag``: the padded window (``window``, float64 on the host),
    its DFT table on the device (``table``) and the magnitudes' row pitch (``ld_mag``: n_bins rounded up to 64, a mel projection's c_in)."""

    def __init__(self, device, n_fft=1024, hop=256, win_length=None, window="hann"):
        check_stft_params(n_fft, hop)
        self.window = padded_window(window, win_length, n_fft)
        self.device = require_cuda(device)
        _abi.load()
        self.n_fft, self.hop = int(n_fft), int(hop)
        self.ld_mag = hip.round_up(self.n_fft // 2 + 1, 64)
        self.table = torch.from_numpy(dft_table(self.window, self.n_fft)).to(self.device)

    def frames(self, pw):
        """-> RaggedBatch over the frames of a ``PackedWaves``"""
        if not pw.lens:
            raise ValueError("no waveform")
        return hip.RaggedBatch([frame_count(n, self.n_fft, self.hop) for n in pw.lens], self.device)

    def magnitude(self, pw, want_pow=False):
        """-> (RaggedBatch over frames, |X| f32 (rows, ld_mag), sum_k |X|^2 f32 (rows,) or None)"""
        rb = self.frames(pw)
        return (rb, *hip.stft_mag(rb, pw.cu, pw.lens, pw.x, self.table, self.n_fft, self.hop, self.ld_mag, want_pow=want_pow))

    @torch.no_grad()
    def energy(self, pw, feat_lengths=None, durations=None):
        """Per utterance sqrt(max(sum_k |X|^2, 1e-10)) (energy.py:69-101); ``feat_lengths``: truncate / zero-pad to these frame counts;
        ``durations`` (one integer sequence per utterance, summing to the adjusted length): token-wise mean of the positive values."""
        rb, _, pow_sum = self.magnitude(pw, True)
        return adjust_and_average(rb, hip.energy_frames(pow_sum), feat_lengths, durations)


class LogMelExtractor:
    """``logmelfilterbank`` of the reference (mel.py:11-73) for a batch of waveforms on the GPU: a ``PackedWaves`` or a list of numpy
    arrays / tensors.  ``stft``: a front end to share (default: one of its own from the STFT parameters).
    ``extractor(waves)`` -> (RaggedBatch over frames, feats f32 (rows, round_up(num_mels, 64)), padding columns zero);
    ``extractor.energy(waves, feat_lengths, durations)`` -> list of per-utterance f32 tensors (``Stft.energy``)."""

    def __init__(self, device, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80,
                 fmin=None, fmax=None, eps=1e-10, log_base=10.0, stft=None):
        try:
            self.log_code = {None: 0, 2.0: 2, 10.0: 10}[None if log_base is None else float(log_base)]
        except (KeyError, TypeError, ValueError):
            raise ValueError(f"{log_base} is not supported.") from None        # the reference's message (mel.py:73)
        self.stft = stft or Stft(device, fft_size, hop_size, win_length, window)
        self.device, self.n_fft, self.hop = self.stft.device, self.stft.n_fft, self.stft.hop
        self.num_mels, self.eps = int(num_mels), float(eps)
        self.ld_out = hip.round_up(self.num_mels, 64)
        mel = mel_filterbank(sampling_rate, self.n_fft, self.num_mels, fmin, fmax)            # (n_bins, n_mels)
        with hip.operands(None):     # exact f32 always
            self.mel_w = hip.PackedConv(torch.from_numpy(mel.T.copy()), None, F32, self.device)     # c_in = stft.ld_mag

    @torch.no_grad()
    def mel(self, waves):
        """-> (RaggedBatch over frames, linear mel spectrogram f32 (rows, num_mels)): np.dot(spc, mel_basis.T) of mel.py:64."""
        rb, mag, _ = self.stft.magnitude(PackedWaves.from_list(waves, self.device))
        return rb, self.mel_w(rb, mag)

    @torch.no_grad()
    def __call__(self, waves):
        rb, mel = self.mel(waves)
        return rb, hip.logmel_post(mel, self.num_mels, self.ld_out, self.eps, self.log_code)

    def energy(self, waves, feat_lengths=None, durations=None):
        return self.stft.energy(PackedWaves.from_list(waves, self.device), feat_lengths, durations)


_extractor = functools.lru_cache(maxsize=16)(LogMelExtractor)


def logmelfilterbank(audio, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=None,
                     fmax=None, eps=1e-10, log_base=10.0):
    """The reference's signature (mel.py:11-23): ndarray (T,) -> float32 ndarray (#frames, num_mels), computed on cuda (the
    current device).  One extractor is kept per parameter set."""
    ex = _extractor("cuda", sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps, log_base)
    _, feats = ex([np.asarray(audio)])
    return feats[:, :num_mels].cpu().numpy()


class Energy:
    """``Energy`` of the reference (energy.py:16-122) on the GPU: ndarray in, float32 ndarray out; ``extract`` is the ragged entry over a
    ``PackedWaves``.  ``center`` / ``normalized`` / ``onesided`` are accepted and, as in the reference (its STFT call does not take
    them), not used.  ``reduction_factor`` must be 1, as every model here requires.  ``stft``: a front end to share (no mel weights)."""

    def __init__(self, fs=22050, n_fft=1024, win_length=None, hop_length=256, window="hann", center=True, normalized=False,
                 onesided=True, use_token_averaged_energy=True, reduction_factor=None, device="cuda", stft=None):
        if reduction_factor != 1 and (use_token_averaged_energy or reduction_factor is not None):
            raise ValueError(f"reduction_factor must be 1 (got {reduction_factor})")
        self.fs, self.n_fft, self.hop_length, self.win_length, self.window = fs, n_fft, hop_length, win_length, window
        self.use_token_averaged_energy, self.reduction_factor = use_token_averaged_energy, reduction_factor
        self.stft = stft or Stft(device, n_fft, hop_length, win_length, window)
        if (self.stft.n_fft, self.stft.hop) != (n_fft, hop_length):
            raise ValueError("Energy: the shared front end has another n_fft / hop_length")

    def output_size(self):
        return 1

    def extract(self, pw, feat_lengths=None, durations=None):
        """The ragged entry: a ``PackedWaves`` -> list of per-utterance f32 device tensors, token-averaged where ``durations`` is given."""
        return self.stft.energy(pw, feat_lengths, durations)

    def forward(self, input, feat_length=None, durations=None):
        if self.use_token_averaged_energy and durations is None:
            raise ValueError("use_token_averaged_energy needs durations")
        e = self.extract(PackedWaves.from_list([np.asarray(input)], self.stft.device), None if feat_length is None else [int(feat_length)],
                         [durations] if self.use_token_averaged_energy else None)
        return e[0].cpu().numpy()
