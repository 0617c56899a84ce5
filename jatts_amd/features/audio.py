"""Audio reading (csrc/resample.hip): ``read_audio`` (``jatts/utils/utils.py:201-234``) with its sample-rate conversion
as a kernel (``Resampler`` / ``resample``, ``jatts_resample``: a Kaiser-windowed-sinc polyphase FIR of this project's own definition, an
exact-f32 MFMA contraction like the STFT).  The converter is pinned exactly on ``scipy.signal.resample_poly`` in float64
(``tests/golden/resample_kat.npz``); parity with ``librosa.load(sr=...)``, whose default is soxr_hq, is UNPINNED: librosa, soxr and
resampy are absent from the build environment."""
import functools
import logging
import math

import numpy as np
import torch

from .. import _abi, hip
from .common import PackedWaves, require_cuda, require_device_tensor

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


class Resampler:
    """Rational sample-rate conversion sr_in -> sr_out on the GPU (``jatts_resample``), taps and table cached on the device.

    ``resampler(waves)``: a list of 1-D float32 DEVICE tensors -> a list of device tensors (views of one buffer), or a ``PackedWaves``
    -> a ``PackedWaves``; utterance b has ceil(n_b * up / down) samples.  sr_in == sr_out returns the input untouched.  The result is
    bit for bit independent of how the utterances are batched."""

    def __init__(self, device, sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
        self.device = require_cuda(device)
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
        out = PackedWaves(torch.empty(sum(n_out), dtype=torch.float32, device=pw.x.device), n_out)
        hip.resample(pw.cu, out.cu, pw.lens, n_out, pw.x, self.table, self.up, self.down, self.half_len, out=out.x)
        return out

    def __call__(self, waves):
        if isinstance(waves, PackedWaves):
            return self.packed(waves)
        waves = list(waves)
        for w in waves:
            require_device_tensor(w, "Resampler takes device tensors")
            if w.dtype != torch.float32 or w.dim() != 1:
                raise ValueError(f"Resampler: 1-D float32 waveforms expected, got {w.dtype} {tuple(w.shape)}")
        if self.identity or not waves:
            return waves
        return self.packed(PackedWaves.from_list(waves, waves[0].device)).split()


_resampler = functools.lru_cache(maxsize=16)(Resampler)


def resample(x, sr_in, sr_out, zeros=RESAMPLE_ZEROS, rolloff=RESAMPLE_ROLLOFF, beta=RESAMPLE_BETA):
    """One-shot form: a 1-D float32 device tensor (or a list of them, or a ``PackedWaves``) at sr_in -> the same at sr_out.  One
    ``Resampler`` is kept per device and parameter set."""
    one = isinstance(x, torch.Tensor)
    first = x if one else (x.x if isinstance(x, PackedWaves) else (x[0] if len(x) else None))
    if first is None:
        return []
    require_device_tensor(first, "resample takes device tensors")
    rs = _resampler(str(first.device), int(sr_in), int(sr_out), int(zeros), float(rolloff), float(beta))
    return rs([x])[0] if one else rs(x)


_NOT_PCM = "{} seems to be different from 16 bit PCM."                       # utils.py:223
_CLIPPING = "{} causes clipping (max: {}). it is better to re-consider global gain scale."      # utils.py:229-230


def read_audio_batch(items, sr, global_gain_scale=1.0, device="cuda"):
    """``read_audio`` for a batch: ``items`` = (wav_path, start, end) per utterance -> a list with, per utterance, a 1-D float32 device
    tensor at ``sr`` or None where the gain clips (the reference's warning is logged).  Files are decoded on the host, grouped by their
    native rate, and each group is ONE upload, ONE ``jatts_resample`` launch and ONE ``jatts_wave_gain_peak`` launch; the peaks of the
    whole batch come back in one read."""
    from ..wavio import decode_wav
    dev = require_cuda(device)
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
    warning) when the gain clips.  A peak above 1 before the gain raises AssertionError in the reference's words.  The file is decoded as
    integer PCM (``wavio.decode_wav``) and converted by ``Resampler``.  Two facts about librosa.load are [recalled], not verifiable
    here: a multi-channel file is reduced to the mean of its channels (mono=True), and ``start`` / ``end`` become sample offsets at the
    file's own rate by truncation (int(offset * sr_native), int(duration * sr_native))."""
    w = read_audio_batch([(wav_path, start, end)], sr, global_gain_scale)[0]
    return None if w is None else w.cpu().numpy()
