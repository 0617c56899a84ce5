"""Stage-1 features of the recipes on the GPU: log-mel filterbank and energy.

Replaces the reference's ``jatts/modules/feature_extract/mel.py:11-73`` (``logmelfilterbank``) and
``feature_extract/energy.py:69-122`` (``Energy.forward``), which run librosa on one CPU thread: the magnitude STFT is one
exact-f32 MFMA contraction over raw samples (``jatts_stft_mag``: reflect padding while the operand is staged, the periodic
Hann window folded into the DFT table), the mel projection a ``jatts_conv1d`` launch, the rest row-wise kernels.

GPU only: a CPU device or a missing library raises ``JattsHipError``.  torch / numpy are used for constant preparation
(window, mel matrix, DFT table) and plumbing, never for the arithmetic.

librosa itself is absent from the build environment, so parity with it is NOT pinned; the tests pin this module on
``torch.stft`` in float64 and on ``transformers.audio_utils.mel_filter_bank(norm="slaney", mel_scale="slaney")``.

Pitch is here too (``Pitch``, the reference's ``feature_extract/dio.py:21-159``): the reference extracts F0 with DIO + StoneMask through
pyworld, which is absent from the build environment, so the raw track comes from an autocorrelation estimator of our own definition
(Boersma 1993 on the STFT's frames: ``jatts_stft_mag`` -> ``jatts_acf_from_mag``, the same exact-f32 MFMA contraction ->
``jatts_pitch_pick``), pinned on a float64 restatement; parity with DIO / StoneMask is UNPINNED.  The steps after the raw track
(continuous F0, log, length adjustment, token average) ARE pinned on the real ``Dio.forward`` (``tests/golden/pitch_post_kat.npz``).

The second half of stage 1 lives here too: ``FeatureStatistics`` is the per-feature ``sklearn.preprocessing.StandardScaler`` of
``jatts/bin/compute_statistics.py:75-103`` as a running float64 state on the device (``jatts_col_moments``: one launch pair per
``partial_fit``, fixed summation order, no read-back before ``finalize``), ``standardize`` the ``StandardScaler.transform`` of
``jatts/datasets/tts_dataset.py:69-145`` (``jatts_standardize``).  These ARE pinned on the real thing: sklearn 1.7.2 wrote
``tests/golden/stats_kat.npz``.  ``python -m jatts_amd.bin.compute_statistics`` is the reference's CLI on top of them.

The first step of stage 1 is here as well: ``read_audio`` (``jatts/utils/utils.py:201-234``) with its sample-rate conversion as a
kernel (``Resampler`` / ``resample``, ``jatts_resample``: a Kaiser-windowed-sinc polyphase FIR of our own definition, an exact-f32
MFMA contraction like the STFT).  The converter is pinned exactly on ``scipy.signal.resample_poly`` in float64
(``tests/golden/resample_kat.npz``); parity with ``librosa.load(sr=...)``, whose default is soxr_hq, is UNPINNED.
``python -m jatts_amd.bin.preprocess`` is the reference's stage-1 CLI on top of all of it.
"""
import functools
import math
import os

import numpy as np
import torch

from . import _abi, hip
from ._abi import F32

_LOG_BASES = {None: 0, 2.0: 2, 10.0: 10}


def _log_base_code(log_base):
    try:
        return _LOG_BASES[None if log_base is None else float(log_base)]
    except (KeyError, TypeError, ValueError):
        raise ValueError(f"{log_base} is not supported.") from None        # the reference's message (mel.py:73)


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


def _check_stft_params(fft_size, hop_size):
    if fft_size % 64 or not 64 <= fft_size <= 2048:
        raise ValueError(f"fft_size {fft_size} must be a multiple of 64, at most 2048")
    if not 1 <= hop_size <= fft_size:
        raise ValueError(f"hop_size {hop_size} must lie in [1, fft_size]")


class LogMelExtractor:
    """``logmelfilterbank`` of the reference (mel.py:11-73) for a batch of waveforms on the GPU.

    ``extractor(waves)`` -> (RaggedBatch over frames, feats f32 (rows, round_up(num_mels, 64)), padding columns zero);
    ``extractor.energy(waves, feat_lengths, durations)`` -> list of per-utterance f32 tensors (energy.py:69-101)."""

    def __init__(self, device, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80,
                 fmin=None, fmax=None, eps=1e-10, log_base=10.0):
        self.log_code = _log_base_code(log_base)
        _check_stft_params(fft_size, hop_size)
        win = padded_window(window, win_length, fft_size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback)")
        _abi.load()
        self.n_fft, self.hop, self.num_mels, self.eps = int(fft_size), int(hop_size), int(num_mels), float(eps)
        self.n_bins = self.n_fft // 2 + 1
        self.ld_mag = hip.round_up(self.n_bins, 64)                 # = the mel projection's padded c_in
        self.ld_out = hip.round_up(self.num_mels, 64)
        self.table = torch.from_numpy(dft_table(win, self.n_fft)).to(self.device)
        mel = mel_filterbank(sampling_rate, self.n_fft, self.num_mels, fmin, fmax)            # (n_bins, n_mels)
        self.mel_w = hip.pack_conv_weight(torch.from_numpy(mel.T.copy()).float().unsqueeze(-1).to(self.device), F32, 64)

    def _stft(self, waves, want_pow):
        if isinstance(waves, PackedWaves):                          # already packed on the device (Resampler's output): no copy
            if not waves.lens:
                raise ValueError("no waveform")
            rb = hip.RaggedBatch([frame_count(n, self.n_fft, self.hop) for n in waves.lens], self.device)
            mag, pw = hip.stft_mag(rb, waves.cu, waves.lens, waves.x, self.table, self.n_fft, self.hop, self.ld_mag, want_pow=want_pow)
            return rb, mag, pw
        ws = [torch.as_tensor(w).reshape(-1) for w in waves]
        if not ws:
            raise ValueError("no waveform")
        ns = [int(w.numel()) for w in ws]
        rb = hip.RaggedBatch([frame_count(n, self.n_fft, self.hop) for n in ns], self.device)
        x = torch.cat([w.to(torch.float32) for w in ws]).to(self.device).contiguous()
        cu = [0]
        for n in ns:
            cu.append(cu[-1] + n)
        mag, pw = hip.stft_mag(rb, hip.h2d(cu, torch.int32, self.device), ns, x, self.table, self.n_fft, self.hop, self.ld_mag,
                               want_pow=want_pow)
        return rb, mag, pw

    @torch.no_grad()
    def mel(self, waves):
        """-> (RaggedBatch over frames, linear mel spectrogram f32 (rows, num_mels)): np.dot(spc, mel_basis.T) of mel.py:64."""
        rb, mag, _ = self._stft(waves, False)
        return rb, hip.conv1d(rb, mag, self.mel_w, self.ld_mag, self.num_mels, 1, dtype=F32)

    @torch.no_grad()
    def __call__(self, waves):
        rb, mel = self.mel(waves)
        return rb, hip.logmel_post(mel, self.num_mels, self.ld_out, self.eps, self.log_code)

    @torch.no_grad()
    def energy(self, waves, feat_lengths=None, durations=None):
        """Per utterance sqrt(max(sum_k |X|^2, 1e-10)); ``feat_lengths``: truncate / zero-pad to these frame counts; ``durations``
        (one integer sequence per utterance, summing to the adjusted length): token-wise mean of the positive values."""
        rb, _, pw = self._stft(waves, True)
        e = hip.energy_frames(pw)
        if feat_lengths is not None:
            if len(feat_lengths) != rb.n_seq or min(int(v) for v in feat_lengths) < 0:
                raise ValueError("feat_lengths: one non-negative length per utterance")
            rb_out = hip.RaggedBatch([int(v) for v in feat_lengths], self.device)
            e, rb = hip.energy_adjust(rb, rb_out, e), rb_out
        if durations is not None:
            if len(durations) != rb.n_seq:
                raise ValueError("durations: one sequence per utterance")
            ds = [np.asarray(torch.as_tensor(d).cpu()).astype(np.int64).reshape(-1) for d in durations]
            cum = []
            for d, n in zip(ds, rb.lens):
                if (d < 0).any() or int(d.sum()) != n:
                    raise ValueError(f"durations sum to {int(d.sum())}, the utterance has {n} frames")    # energy.py:104
                cum.extend(int(v) for v in np.cumsum(d))
            rb_tok = hip.RaggedBatch([len(d) for d in ds], self.device)
            e, rb = hip.token_average(rb_tok, rb, hip.h2d(cum or [0], torch.int32, self.device), e), rb_tok
        return [e[rb.cu_host[b]:rb.cu_host[b + 1]] for b in range(rb.n_seq)]


@functools.lru_cache(maxsize=16)
def _extractor(device, sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps, log_base):
    return LogMelExtractor(device, sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps, log_base)


def logmelfilterbank(audio, sampling_rate, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=None,
                     fmax=None, eps=1e-10, log_base=10.0):
    """The reference's signature (mel.py:11-23): ndarray (T,) -> float32 ndarray (#frames, num_mels), computed on cuda (the
    current device).  One extractor is kept per parameter set."""
    ex = _extractor("cuda", sampling_rate, fft_size, hop_size, win_length, window, num_mels, fmin, fmax, eps, log_base)
    _, feats = ex([np.asarray(audio)])
    return feats[:, :num_mels].cpu().numpy()


class Energy:
    """``Energy`` of the reference (energy.py:16-122) on the GPU: ndarray in, float32 ndarray out.  ``center`` / ``normalized`` /
    ``onesided`` are accepted and, as in the reference (its STFT call does not take them), not used.  ``reduction_factor`` must be 1,
    as every model here requires."""

    def __init__(self, fs=22050, n_fft=1024, win_length=None, hop_length=256, window="hann", center=True, normalized=False,
                 onesided=True, use_token_averaged_energy=True, reduction_factor=None, device="cuda"):
        if reduction_factor != 1 and (use_token_averaged_energy or reduction_factor is not None):
            raise ValueError(f"reduction_factor must be 1 (got {reduction_factor})")
        self.fs, self.n_fft, self.hop_length, self.win_length, self.window = fs, n_fft, hop_length, win_length, window
        self.use_token_averaged_energy, self.reduction_factor = use_token_averaged_energy, reduction_factor
        self._ex = LogMelExtractor(device, fs, n_fft, hop_length, win_length, window)

    def output_size(self):
        return 1

    def forward(self, input, feat_length=None, durations=None):
        if self.use_token_averaged_energy and durations is None:
            raise ValueError("use_token_averaged_energy needs durations")
        e = self._ex.energy([np.asarray(input)], None if feat_length is None else [int(feat_length)],
                            [durations] if self.use_token_averaged_energy else None)
        return e[0].cpu().numpy()


# ---- stage-1 statistics and normalisation (csrc/stats.hip)
STATS_ROWS_PER_GROUP = _abi.STATS_ROWS_PER_GROUP      # rows per summation group of jatts_col_moments (the library's compile-time constant)


def stats_from_state(n, mean, m2):
    """(n, mean, M2) per column -> float64 ``(mean_, var_, scale_)`` as ``StandardScaler.partial_fit`` leaves them (sklearn 1.7.2,
    preprocessing/_data.py): var = M2 / n; scale = sqrt(var), except that a column which cannot be told from a constant one gets
    scale 1.0 -- ``_is_constant_feature``: var <= n eps var + (n mean eps)^2 with eps = float64's, the error bound of the two-pass
    variance; ``_handle_zeros_in_scale`` with that mask.  Pure numpy.  Raises ValueError for a non-finite state or an empty one."""
    n = np.atleast_1d(np.asarray(n, dtype=np.float64))
    mean = np.atleast_1d(np.asarray(mean, dtype=np.float64))
    m2 = np.atleast_1d(np.asarray(m2, dtype=np.float64))
    n = np.broadcast_to(n, mean.shape)
    if not (np.isfinite(n).all() and np.isfinite(mean).all() and np.isfinite(m2).all()):
        raise ValueError("statistics state is not finite (NaN or infinity in the features: they are not skipped)")
    if (n <= 0).any():
        raise ValueError("statistics of zero samples")
    var = m2 / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return mean.copy(), var, scale


_H5_ERROR = "{} .h5 stats needs h5py; convert to .npz (<feat>_mean, <feat>_scale)"


def save_stats(path, feat_name, mean, scale):
    """Write or update ``<feat_name>_mean`` / ``<feat_name>_scale`` (float32) in ``path`` (compute_statistics.py:94-103): .npz always
    (the twin format ``bin.tts_decode.read_stats`` reads; other entries of an existing file are kept), .h5 through h5py."""
    path = str(path)
    new = {f"{feat_name}_mean": np.asarray(mean).astype(np.float32), f"{feat_name}_scale": np.asarray(scale).astype(np.float32)}
    if path.endswith(".npz"):
        old = {}
        if os.path.exists(path):
            with np.load(path) as z:
                old = {k: z[k] for k in z.files}
        old.update(new)
        with open(path, "wb") as f:        # (np.savez appends ".npz" to a bare name; an open file is taken as it is)
            np.savez(f, **old)
        return
    try:
        import h5py
    except ImportError as e:
        raise ImportError(_H5_ERROR.format("writing")) from e
    with h5py.File(path, "a") as f:
        for k, v in new.items():
            if k in f:
                del f[k]
            f.create_dataset(k, data=v)


class FeatureStatistics:
    """One ``sklearn.preprocessing.StandardScaler`` of compute_statistics.py:81-92 as a running float64 state on the GPU.

    ``partial_fit`` / ``partial_fit_ragged`` / ``merge`` launch kernels and return; nothing is read back until ``finalize()``, the
    one synchronisation.  The state (``self.state``, float64 (3, dim): samples seen | mean | M2) is bit-identical from run to run for
    the same sequence of calls.  Unlike sklearn, NaN values are NOT skipped: they (and infinities) make ``finalize`` raise."""

    def __init__(self, dim, device="cuda"):
        self.dim = int(dim)
        if self.dim < 1:
            raise ValueError(f"dim {dim} must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback)")
        _abi.load()
        self.state = torch.zeros(3, self.dim, dtype=torch.float64, device=self.device)
        self._ws = torch.empty(2 * self.dim * 8, dtype=torch.float64, device=self.device)     # own scratch: grows, never shared

    def _fit(self, x, ld, rows):
        need = hip.col_moments_ws_doubles(rows, self.dim)
        if need > self._ws.numel():
            self._ws = torch.empty(2 * need, dtype=torch.float64, device=self.device)         # (stream-ordered: the old one may still be read)
        hip.col_moments(x, ld, self.dim, rows, self.state, self._ws)
        return self

    @torch.no_grad()
    def partial_fit(self, x, ld=None):
        """x: device f32 (rows, ld) with ld >= dim (columns dim.. are ignored), or (rows,) when dim == 1.  ``ld`` overrides the row
        pitch of a flat buffer."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback): partial_fit takes a device tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"partial_fit: float32 expected, got {x.dtype}")
        if ld is None:
            if x.dim() == 1 and self.dim == 1:
                ld = 1
            elif x.dim() == 2:
                ld = x.shape[1]
            else:
                raise ValueError(f"partial_fit: (rows, ld) expected, got {tuple(x.shape)}")
        ld = int(ld)
        if ld < self.dim or x.numel() % ld:
            raise ValueError(f"partial_fit: {tuple(x.shape)} is not (rows, ld = {ld}) with ld >= dim = {self.dim}")
        return self._fit(x.contiguous(), ld, x.numel() // ld)

    def partial_fit_ragged(self, rb, feats):
        """What ``LogMelExtractor.__call__`` returns: the packed rows of all utterances of the batch are ONE partial_fit call."""
        if feats.dim() != 2 or feats.shape[0] != rb.total:
            raise ValueError("partial_fit_ragged: feats must hold the batch's packed rows")
        return self.partial_fit(feats)

    @torch.no_grad()
    def merge(self, other):
        """Fold another accumulator (a shard of the same dataset) into this one; ``other`` is left as it is."""
        if not isinstance(other, FeatureStatistics) or other.dim != self.dim or other is self:
            raise ValueError("merge: another FeatureStatistics of the same dim expected")
        hip.col_moments_merge(self.state, other.state.to(self.device))
        return self

    def finalize(self):
        """The one synchronisation: float64 numpy ``mean_``, ``var_``, ``scale_`` (dim,) and ``n_samples_seen_`` (int) as attributes
        and as the returned tuple.  ValueError when the state is not finite or empty."""
        st = self.state.cpu().numpy()
        self.mean_, self.var_, self.scale_ = stats_from_state(st[0], st[1], st[2])
        self.n_samples_seen_ = int(st[0][0])
        return self.mean_, self.var_, self.scale_, self.n_samples_seen_

    def save(self, path, feat_name):
        """finalize() and write ``<feat_name>_mean`` / ``<feat_name>_scale`` as float32 (see ``save_stats``)."""
        mean, _, scale, _ = self.finalize()
        save_stats(path, feat_name, mean, scale)


@torch.no_grad()
def standardize(x, mean, scale, dim=None):
    """``StandardScaler.transform`` (tts_dataset.py:69-145) on the GPU: device f32 x (rows, ld) -> (x - mean) / scale on the first
    ``dim`` columns (default: len(mean)), one f32 subtract and one f32 divide, both correctly rounded; columns dim.. are zero.
    ``mean`` / ``scale``: numpy or tensors, cast to float32 as the stats file stores them."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback): standardize takes a device tensor")
    m = torch.as_tensor(np.asarray(mean, dtype=np.float32) if not isinstance(mean, torch.Tensor) else mean).to(torch.float32).reshape(-1)
    s = torch.as_tensor(np.asarray(scale, dtype=np.float32) if not isinstance(scale, torch.Tensor) else scale).to(torch.float32).reshape(-1)
    dim = int(m.numel()) if dim is None else int(dim)
    if m.numel() != s.numel() or not 1 <= dim <= m.numel():
        raise ValueError("standardize: mean and scale must have the same length >= dim")
    x2 = x.reshape(-1, 1) if x.dim() == 1 else x
    if x2.dim() != 2 or x2.shape[1] < dim or x2.dtype != torch.float32:
        raise ValueError(f"standardize: float32 (rows, ld >= {dim}) expected, got {x.dtype} {tuple(x.shape)}")
    y = hip.standardize(x2.contiguous(), m.to(x.device).contiguous(), s.to(x.device).contiguous(), dim)
    return y.reshape(-1) if x.dim() == 1 else y


# ---- sample-rate conversion and read_audio (csrc/resample.hip)
# The converter is this project's own: a Kaiser-windowed-sinc polyphase FIR.  Its arithmetic is pinned exactly on
# scipy.signal.resample_poly in float64 (tests/golden/resample_kat.npz).  Parity with librosa.load(sr=...), whose default is soxr_hq,
# is UNPINNED: librosa, soxr and resampy are absent from the build environment.
RESAMPLE_ZEROS = 64                          # zero crossings of the sinc a side, per unit of max(up, down)
RESAMPLE_ROLLOFF = 0.9475937167399596        # cutoff as a share of the lower Nyquist  } the published "kaiser_best" constants [recalled,
RESAMPLE_BETA = 14.769656459379492           # Kaiser window parameter                 } not verifiable here]
RESAMPLE_MAX_K, RESAMPLE_MAX_NBP, RESAMPLE_MAX_TABLE_BYTES = 2048, 512, 4 << 20


def resample_ratio(sr_in, sr_out):
    """(up, down) in lowest terms for integer sampling rates."""
    if int(sr_in) != sr_in or int(sr_out) != sr_out or sr_in < 1 or sr_out < 1:
        raise ValueError(f"sampling rates must be positive integers (got {sr_in} -> {sr_out})")
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def resample_taps(sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
    """float32 (2 * half_len + 1,), half_len = zeros * max(up, down): up * firwin(2 * half_len + 1, rolloff / max(up, down),
    window=("kaiser", beta)), restated from the formula -- sinc low-pass times the symmetric Kaiser window (np.i0), scaled to unit gain
    at DC -- designed in float64 and rounded ONCE.  zeros=10, rolloff=1, beta=5 is scipy.signal.resample_poly's own default design
    (-14 dB just above the Nyquist frequency: not ours)."""
    return resample_design(sr_in, sr_out, zeros, rolloff, beta).astype(np.float32)


def resample_design(sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
    """The float64 design ``resample_taps`` rounds."""
    up, down = resample_ratio(sr_in, sr_out)
    m_rate = max(up, down)
    zeros = int(zeros)
    if up == down or zeros < 1 or not 0.0 < rolloff / m_rate < 1.0 or beta < 0.0:
        raise ValueError(f"no filter for {sr_in} -> {sr_out} with zeros={zeros}, rolloff={rolloff}, beta={beta}")
    half_len = zeros * m_rate
    m = np.arange(-half_len, half_len + 1, dtype=np.float64)
    cutoff = float(rolloff) / m_rate
    h = cutoff * np.sinc(cutoff * m)
    h *= np.i0(float(beta) * np.sqrt(1.0 - (m / half_len) ** 2)) / np.i0(float(beta))
    h /= h.sum()
    return up * h


def resample_out_len(n_in, up, down):
    """ceil(n_in * up / down)"""
    return -(-int(n_in) * up // down)


def resample_geometry(up, down, half_len):
    """The block form the kernel runs (include/jatts_hip.h: jatts_resample) -> dict r, Nb, Nbp, hop_b, L, K.  A block is Nb = up * r
    consecutive outputs (r = ceil(32 / up) for up < 32, else 1), so every block meets the taps in the same phase pattern, and advances
    hop_b = down * r input samples; L = half_len // up input samples precede its first output's centre; K input samples feed it."""
    r = -(-32 // up) if up < 32 else 1
    nb, hop_b, lead = up * r, down * r, half_len // up
    k = hip.round_up(((nb - 1) * down + half_len) // up + lead + 1, 64)
    return dict(r=r, Nb=nb, Nbp=hip.round_up(nb, 32), hop_b=hop_b, L=lead, K=k)


def resample_table(taps, up, down):
    """float32 (K, Nbp): W[i][c] = taps[c * down - (i - L) * up + half_len] where that index is in range and c < Nb, else 0 -- pure
    indexing of the f32 taps, no arithmetic.  ValueError beyond the kernel's limits."""
    taps = np.asarray(taps, dtype=np.float32)
    if taps.ndim != 1 or taps.size % 2 != 1 or taps.size < 3:
        raise ValueError("taps: an odd number (2 * half_len + 1) expected")
    half_len = taps.size // 2
    g = resample_geometry(up, down, half_len)
    if g["K"] > RESAMPLE_MAX_K:
        raise ValueError(f"resampling {up}/{down} with {taps.size} taps needs K = {g['K']} input samples per block: the limit is K <= {RESAMPLE_MAX_K}")
    if g["Nbp"] > RESAMPLE_MAX_NBP:
        raise ValueError(f"resampling {up}/{down} needs Nbp = {g['Nbp']} table columns: the limit is Nbp <= {RESAMPLE_MAX_NBP}")
    if g["K"] * g["Nbp"] * 4 > RESAMPLE_MAX_TABLE_BYTES:
        raise ValueError(f"resampling {up}/{down} needs a table of {g['K'] * g['Nbp'] * 4} bytes: the limit is {RESAMPLE_MAX_TABLE_BYTES} bytes (4 MiB)")
    i = np.arange(g["K"], dtype=np.int64)[:, None]
    c = np.arange(g["Nbp"], dtype=np.int64)[None, :]
    j = c * down - (i - g["L"]) * up + half_len
    ok = (j >= 0) & (j < taps.size) & (c < g["Nb"])
    return np.where(ok, taps[np.clip(j, 0, taps.size - 1)], np.float32(0.0)).astype(np.float32)


def seconds_to_samples(start, end, sr_native):
    """read_audio's ``start`` / ``end`` (seconds; utils.py:204-209: offset = start, duration = end - start) -> (first sample, number of
    samples) at the file's own rate, both by truncation: int(offset * sr), int(duration * sr), what librosa.load does [recalled].
    Either being None reads the whole file: (0, None)."""
    if start is None or end is None:
        return 0, None
    offset, duration = float(start), float(end) - float(start)
    if offset < 0.0 or duration < 0.0:
        raise ValueError(f"start {start} / end {end}: a non-negative offset and duration expected")
    return int(offset * sr_native), int(duration * sr_native)


class PackedWaves:
    """A ragged batch of waveforms in one device buffer: ``x`` f32 (sum(lens),), ``lens`` on the host, ``cu`` their exclusive scan on the
    device.  What ``Resampler`` returns for such an input and ``LogMelExtractor`` consumes without a copy."""

    def __init__(self, x, lens):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback): PackedWaves takes a device tensor")
        self.lens = [int(v) for v in lens]
        if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.numel() != sum(self.lens) or min(self.lens, default=0) < 0:
            raise ValueError("PackedWaves: a contiguous 1-D float32 buffer of sum(lens) samples expected")
        self.x = x
        self.cu_host = [0]
        for n in self.lens:
            self.cu_host.append(self.cu_host[-1] + n)
        self.cu = hip.h2d(self.cu_host, torch.int32, x.device)

    @classmethod
    def from_list(cls, waves, device):
        ws = [torch.as_tensor(w).reshape(-1).to(torch.float32) for w in waves]
        return cls(torch.cat(ws).to(device).contiguous(), [int(w.numel()) for w in ws])

    def split(self):
        """list of per-utterance views of ``x``"""
        return [self.x[a:b] for a, b in zip(self.cu_host[:-1], self.cu_host[1:])]


class Resampler:
    """Rational sample-rate conversion sr_in -> sr_out on the GPU (``jatts_resample``), taps and table cached on the device.

    ``resampler(waves)``: a list of 1-D float32 DEVICE tensors -> a list of device tensors (views of one buffer), or a ``PackedWaves``
    -> a ``PackedWaves``; utterance b has ceil(n_b * up / down) samples.  sr_in == sr_out returns the input untouched.  The result is
    bit for bit independent of how the utterances are batched.  Pinned on scipy.signal.resample_poly with these taps; parity with
    librosa.load(sr=...) (soxr_hq) is UNPINNED."""

    def __init__(self, device, sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback)")
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = resample_ratio(sr_in, sr_out)
        self.identity = self.up == self.down
        if self.identity:
            return
        taps = resample_taps(sr_in, sr_out, zeros, rolloff, beta)
        self.half_len = taps.size // 2
        self.geometry = resample_geometry(self.up, self.down, self.half_len)
        table = resample_table(taps, self.up, self.down)
        _abi.load()
        self.taps = torch.from_numpy(taps).to(self.device)
        self.table = torch.from_numpy(table).to(self.device)

    def out_len(self, n_in):
        return int(n_in) if self.identity else resample_out_len(n_in, self.up, self.down)

    @torch.no_grad()
    def packed(self, pw):
        if not isinstance(pw, PackedWaves):
            raise TypeError("Resampler.packed takes a PackedWaves")
        if self.identity:
            return pw
        n_out = [self.out_len(n) for n in pw.lens]
        cu_out = [0]
        for n in n_out:
            cu_out.append(cu_out[-1] + n)
        y = hip.resample(pw.cu, hip.h2d(cu_out, torch.int32, pw.x.device), pw.lens, n_out, pw.x, self.table, self.up, self.down,
                         self.half_len)
        return PackedWaves(y, n_out)

    def __call__(self, waves):
        if isinstance(waves, PackedWaves):
            return self.packed(waves)
        waves = list(waves)
        for w in waves:
            if not isinstance(w, torch.Tensor) or not w.is_cuda:
                raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback): Resampler takes device tensors")
            if w.dtype != torch.float32 or w.dim() != 1:
                raise ValueError(f"Resampler: 1-D float32 waveforms expected, got {w.dtype} {tuple(w.shape)}")
        if self.identity or not waves:
            return waves
        return self.packed(PackedWaves(torch.cat(waves).contiguous(), [int(w.numel()) for w in waves])).split()


@functools.lru_cache(maxsize=16)
def _resampler(device, sr_in, sr_out, zeros, rolloff, beta):
    return Resampler(device, sr_in, sr_out, zeros, rolloff, beta)


def resample(x, sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
    """One-shot form: a 1-D float32 device tensor (or a list of them, or a ``PackedWaves``) at sr_in -> the same at sr_out.  One
    ``Resampler`` is kept per device and parameter set."""
    one = isinstance(x, torch.Tensor)
    first = x if one else (x.x if isinstance(x, PackedWaves) else (x[0] if len(x) else None))
    if first is not None and (not isinstance(first, torch.Tensor) or not first.is_cuda):
        raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback): resample takes device tensors")
    if first is None:
        return []
    rs = _resampler(str(first.device), int(sr_in), int(sr_out), int(zeros), float(rolloff), float(beta))
    return rs([x])[0] if one else rs(x)


_NOT_PCM = "{} seems to be different from 16 bit PCM."                       # utils.py:223
_CLIPPING = "{} causes clipping (max: {}). it is better to re-consider global gain scale."      # utils.py:229-230


def read_audio_batch(items, sr, global_gain_scale=1.0, device="cuda"):
    """``read_audio`` for a batch: ``items`` = (wav_path, start, end) per utterance -> a list with, per utterance, a 1-D float32 device
    tensor at ``sr`` or None where the gain clips (the reference's warning is logged).  Files are decoded on the host, grouped by their
    native rate, and each group is ONE upload, ONE ``jatts_resample`` launch and ONE ``jatts_wave_gain_peak`` launch; the peaks of the
    whole batch come back in one read."""
    import logging

    from .wavio import decode_wav
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback)")
    groups = {}
    for idx, (path, start, end) in enumerate(items):
        a, rate = decode_wav(path)
        a = a[:, 0] if a.shape[1] == 1 else a.mean(axis=1, dtype=np.float32)          # mono=True: the channels' mean [recalled]
        first, count = seconds_to_samples(start, end, rate)
        a = a[first:] if count is None else a[first:first + count]
        if a.size == 0:
            raise ValueError(f"{path}: no samples between start {start} and end {end}")
        groups.setdefault(rate, []).append((idx, np.ascontiguousarray(a, dtype=np.float32)))
    out, runs = [None] * len(items), []
    for rate, members in groups.items():
        pw = PackedWaves(torch.from_numpy(np.concatenate([a for _, a in members])).pin_memory().to(dev, non_blocking=True),
                         [a.size for _, a in members])
        rs = _resampler(str(dev), int(rate), int(sr), RESAMPLE_ZEROS, RESAMPLE_ROLLOFF, RESAMPLE_BETA)
        pw = rs.packed(pw)
        runs.append((members, pw, hip.wave_gain_peak(pw.cu, len(members), pw.x, global_gain_scale)))
    for members, pw, peak in runs:
        peak = peak.cpu().numpy()
        for (idx, _), w, (before, after) in zip(members, pw.split(), peak):
            path = items[idx][0]
            if not before <= 1.0:
                raise AssertionError(_NOT_PCM.format(path))
            if not after <= 1.0:
                logging.warning(_CLIPPING.format(path, after))
                continue
            out[idx] = w
    return out


def read_audio(wav_path, sr, start=None, end=None, global_gain_scale=1.0):
    """The reference's ``read_audio`` (jatts/utils/utils.py:201-234), computed on cuda (the current device): the file between ``start``
    and ``end`` (seconds; both or neither) at ``sr``, times ``global_gain_scale`` -> float32 ndarray, or None (with the reference's
    warning) when the gain clips.  A peak above 1 before the gain raises AssertionError in the reference's words.

    The file is decoded as integer PCM (``wavio.decode_wav``); the sample-rate conversion is ``Resampler``'s -- pinned on
    scipy.signal.resample_poly, parity with librosa.load(sr=...) (soxr_hq) UNPINNED.  Two facts about librosa.load are [recalled],
    not verifiable here: a multi-channel file is reduced to the mean of its channels (mono=True), and ``start`` / ``end`` become sample
    offsets at the file's own rate by truncation (int(offset * sr_native), int(duration * sr_native))."""
    w = read_audio_batch([(wav_path, start, end)], sr, global_gain_scale)[0]
    return None if w is None else w.cpu().numpy()


# ---- pitch (csrc/pitch.hip)
# The estimator is this project's own: Boersma's 1993 autocorrelation method on the STFT's frames (the definition is written out in
# csrc/pitch.hip and DESIGN §7 f.8), pinned on a float64 restatement (tests/pitch_reference.py).  Parity with the reference's DIO +
# StoneMask (pyworld, absent from the build environment) is UNPINNED.  The steps after the raw track -- continuous F0, log, length
# adjustment, token average -- ARE pinned on the real Dio.forward (tests/golden/pitch_post_kat.npz).
PITCH_VOICING_THRESHOLD, PITCH_SILENCE_THRESHOLD, PITCH_OCTAVE_COST = 0.45, 0.03, 0.01      # Boersma's defaults


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
    entry over a ``PackedWaves``.  One table pair (windowed DFT, autocorrelation) is kept per (f0min, f0max).  Parity of the raw track
    with DIO / StoneMask is UNPINNED; everything after it follows ``Dio.forward`` and is pinned on it."""

    def __init__(self, fs=22050, n_fft=1024, hop_length=256, use_token_averaged_f0=True, use_continuous_f0=True, use_log_f0=True,
                 reduction_factor=None, voicing_threshold=PITCH_VOICING_THRESHOLD, silence_threshold=PITCH_SILENCE_THRESHOLD,
                 octave_cost=PITCH_OCTAVE_COST, device="cuda"):
        if use_token_averaged_f0 and not (reduction_factor is not None and reduction_factor >= 1):
            raise ValueError(f"use_token_averaged_f0 needs reduction_factor >= 1 (got {reduction_factor})")      # dio.py:58-59
        _check_stft_params(n_fft, hop_length)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.JattsHipError("jatts_amd.features runs on the GPU only (no CPU fallback)")
        _abi.load()
        self.fs, self.n_fft, self.hop_length = fs, int(n_fft), int(hop_length)
        self.use_token_averaged_f0, self.use_continuous_f0, self.use_log_f0 = use_token_averaged_f0, use_continuous_f0, use_log_f0
        self.reduction_factor = reduction_factor
        self.voicing_threshold, self.silence_threshold, self.octave_cost = float(voicing_threshold), float(silence_threshold), float(octave_cost)
        self.ld_mag = hip.round_up(self.n_fft // 2 + 1, 64)
        self._tables = {}

    def output_size(self):
        return 1

    def get_parameters(self):
        return dict(fs=self.fs, n_fft=self.n_fft, hop_length=self.hop_length, use_token_averaged_f0=self.use_token_averaged_f0,
                    use_continuous_f0=self.use_continuous_f0, use_log_f0=self.use_log_f0, reduction_factor=self.reduction_factor)

    def tables(self, f0min, f0max):
        """(lo, hi, sum w^2, windowed DFT table, autocorrelation table) of a range, built once."""
        key = (float(f0min), float(f0max))
        hit = self._tables.get(key)
        if hit is None:
            lo, hi, w_len = pitch_geometry(self.fs, self.n_fft, f0min, f0max)
            win = padded_window("hann", w_len, self.n_fft)
            hit = (lo, hi, float(np.dot(win, win)), torch.from_numpy(dft_table(win, self.n_fft)).to(self.device),
                   torch.from_numpy(acf_table(win, self.n_fft, hi)).to(self.device))
            self._tables[key] = hit
        return hit

    @torch.no_grad()
    def raw(self, waves, f0min, f0max, peaks=None):
        """Steps 1-5 over a ``PackedWaves`` -> (RaggedBatch over frames, f0 f32 (rows,) with 0 for unvoiced frames, tau int32 (rows,)).
        ``peaks``: device f32 (n_seq,) max |x| per utterance (default: one ``jatts_wave_gain_peak`` launch with gain 1)."""
        if not isinstance(waves, PackedWaves):
            raise TypeError("Pitch.raw takes a PackedWaves")
        if not waves.lens:
            raise ValueError("no waveform")
        lo, hi, sum_w2, dft, acf = self.tables(f0min, f0max)
        rb = hip.RaggedBatch([frame_count(n, self.n_fft, self.hop_length) for n in waves.lens], self.device)
        if peaks is None:
            peak, stride = hip.wave_gain_peak(waves.cu, len(waves.lens), waves.x, 1.0), 2      # (x * 1.0: the samples keep their bits)
        else:
            peak, stride = peaks.to(torch.float32).contiguous(), 1
        mag, _ = hip.stft_mag(rb, waves.cu, waves.lens, waves.x, dft, self.n_fft, self.hop_length, self.ld_mag)
        r = hip.acf_from_mag(rb, mag, acf)
        f0, tau = hip.pitch_pick(rb, r, peak, stride, lo, hi, self.fs, f0min, sum_w2, self.voicing_threshold, self.silence_threshold,
                                 self.octave_cost)
        return rb, f0, tau

    @torch.no_grad()
    def post(self, rb, f0, feat_lengths=None, durations=None):
        """Step 6 on a raw track (dio.py:110-159) -> list of per-utterance f32 device tensors."""
        p = hip.f0_continuous_log(rb, f0, self.use_continuous_f0, self.use_log_f0)
        if feat_lengths is not None:
            if len(feat_lengths) != rb.n_seq or min(int(v) for v in feat_lengths) < 0:
                raise ValueError("feat_lengths: one non-negative length per utterance")
            rb_out = hip.RaggedBatch([int(v) for v in feat_lengths], self.device)
            p, rb = hip.energy_adjust(rb, rb_out, p), rb_out
        if self.use_token_averaged_f0:
            if durations is None or len(durations) != rb.n_seq:
                raise ValueError("use_token_averaged_f0 needs durations: one sequence per utterance")
            ds = [np.asarray(torch.as_tensor(d).cpu()).astype(np.int64).reshape(-1) * int(self.reduction_factor) for d in durations]
            cum = []
            for d, n in zip(ds, rb.lens):
                if (d < 0).any() or not 0 <= n - int(d.sum()) < self.reduction_factor:
                    raise ValueError(f"durations sum to {int(d.sum())}, the utterance has {n} frames")      # dio.py:149
                cum.extend(int(v) for v in np.cumsum(d))
            rb_tok = hip.RaggedBatch([len(d) for d in ds], self.device)
            p, rb = hip.token_average(rb_tok, rb, hip.h2d(cum or [0], torch.int32, self.device), p), rb_tok
        return [p[rb.cu_host[b]:rb.cu_host[b + 1]] for b in range(rb.n_seq)]

    def extract(self, waves, f0min, f0max, feat_lengths=None, durations=None, peaks=None):
        """The ragged entry: a ``PackedWaves`` of utterances that share one f0 range -> list of per-utterance f32 device tensors."""
        rb, f0, _ = self.raw(waves, f0min, f0max, peaks)
        return self.post(rb, f0, feat_lengths, durations)

    def forward(self, input, f0min=80, f0max=400, feat_length=None, durations=None):
        pw = PackedWaves.from_list([np.asarray(input)], self.device)
        out = self.extract(pw, f0min, f0max, None if feat_length is None else [int(feat_length)],
                           [durations] if self.use_token_averaged_f0 else None)
        return out[0].cpu().numpy()
