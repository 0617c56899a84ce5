"""Stage-1 features of the recipes on the GPU: log-mel filterbank and energy.

Replaces the reference's ``jatts/modules/feature_extract/mel.py:11-73`` (``logmelfilterbank``) and
``feature_extract/energy.py:69-122`` (``Energy.forward``), which run librosa on one CPU thread: the magnitude STFT is one
exact-f32 MFMA contraction over raw samples (``jatts_stft_mag``: reflect padding while the operand is staged, the periodic
Hann window folded into the DFT table), the mel projection a ``jatts_conv1d`` launch, the rest row-wise kernels.

GPU only: a CPU device or a missing library raises ``JattsHipError``.  torch / numpy are used for constant preparation
(window, mel matrix, DFT table) and plumbing, never for the arithmetic.

librosa itself is absent from the build environment, so parity with it is NOT pinned; the tests pin this module on
``torch.stft`` in float64 and on ``transformers.audio_utils.mel_filter_bank(norm="slaney", mel_scale="slaney")``.
Pitch (WORLD / DIO) stays out of scope.

The second half of stage 1 lives here too: ``FeatureStatistics`` is the per-feature ``sklearn.preprocessing.StandardScaler`` of
``jatts/bin/compute_statistics.py:75-103`` as a running float64 state on the device (``jatts_col_moments``: one launch pair per
``partial_fit``, fixed summation order, no read-back before ``finalize``), ``standardize`` the ``StandardScaler.transform`` of
``jatts/datasets/tts_dataset.py:69-145`` (``jatts_standardize``).  These ARE pinned on the real thing: sklearn 1.7.2 wrote
``tests/golden/stats_kat.npz``.  ``python -m jatts_amd.bin.compute_statistics`` is the reference's CLI on top of them.
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
