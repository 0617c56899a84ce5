"""Stage 5, objective evaluation (csrc/evaluate.hip): the reference's ``jatts/evaluate/dtw_based.py`` -- MCD, F0RMSE, F0CORR
and DDUR of a generated wave against its ground truth -- for batches of pairs on the GPU.  The reference's stage needs pyworld, pysptk,
fastdtw and librosa, all absent from the build environment, so the arithmetic is of this project's own definition:

  frames   hop = round(fs * 0.005), centred reflect-padded frames (``Stft``)
  cepstra  orthonormal DCT-II (coefficients 0..39) of the natural-log mel spectrum, 80 bins from 70 Hz to fs / 2, fft 1024
  VAD      frames whose power sum exceeds 10^-2 of the utterance's mean (npow > -20 dB), decided in float64 without a logarithm
  DTW      EXACT dynamic time warping on Euclidean distances, float64 accumulation, ties to the diagonal, then (i - 1, j), then (i, j - 1)
  MCD      mean over the path of 10 / ln 10 * sqrt(2 sum_c (a_i[c] - b_j[c])^2), c0 included
  F0       ``Pitch.raw`` (fft 2048) at the same hop; a second DTW on the cepstra of the voiced frames; RMSE and Pearson's r over its path
  DDUR     |trimmed length of x - of y| / fs, the trim keeping the frames of an Stft(2048, 512) within 60 dB of the wave's maximum

PINNED: every kernel on a float64 / exact restatement (tests/evaluate_reference.py).  UNPINNED: parity of the numbers with the
reference's WORLD mel-cepstra, Harvest F0, fastdtw (an approximation of the exact DTW built here) and librosa.effects.trim.  MCD values
from here are comparable between systems evaluated here, NOT with values the reference prints.

torch is plumbing: buffers, the stream and two device-to-host reads per batch (the selection counts that size the DTW, the final sums)."""
import logging
import math

import numpy as np
import torch

from . import hip
from ._abi import F32
from .features.common import PackedWaves, require_cuda, require_device_tensor
from .features.pitch import Pitch
from .features.stft import LogMelExtractor, Stft

MCEP_DIM, MCEP_SHIFT_MS, MCEP_FFTL = 39, 5, 1024           # jatts/utils/signal.py
N_MELS, MEL_FMIN, F0_FFT, TRIM_FFT, TRIM_HOP, TRIM_TOP_DB, VAD_DB = 80, 70.0, 2048, 2048, 512, 60.0, -20.0
MCD_SCALE = 10.0 / math.log(10.0)
DEFINITIONS = ("MCD / F0RMSE / F0CORR / DDUR are of jatts_amd's own definition (log-mel DCT cepstra, autocorrelation F0, exact DTW, "
               "60 dB power trim): pinned on float64 restatements, NOT on the reference's WORLD / Harvest / fastdtw / librosa -- compare "
               "them between systems evaluated here, not with numbers the reference prints")
NO_F0_WARNING = ("No nonzero f0 is found. Skip f0rmse f0corr computation and set them to NaN. "
                 "This might due to unconverge training. Please tune the training time and hypers.")      # dtw_based.py:56-62
log = logging.getLogger(__name__)


def dct_matrix(n_in=N_MELS, n_out=MCEP_DIM + 1):
    """float64 (n_out, n_in): the orthonormal DCT-II, row c = s_c cos(pi (k + 1/2) c / n_in), s_0 = sqrt(1 / n_in), else sqrt(2 / n_in)."""
    k = np.arange(n_in, dtype=np.float64)[None, :]
    c = np.arange(n_out, dtype=np.float64)[:, None]
    w = np.cos(np.pi * (k + 0.5) * c / n_in) * math.sqrt(2.0 / n_in)
    w[0] *= math.sqrt(0.5)
    return w


def metrics_from_sums(mcd_sums, f0_sums):
    """The eight float64 sums of ``hip.dtw_path_stats`` over the power path and over the F0 path (None: no voiced frame on a side) ->
    (MCD, F0RMSE, F0CORR); Pearson's r from the moments."""
    mcd = MCD_SCALE * mcd_sums[1] / mcd_sums[0]
    if f0_sums is None:
        return mcd, math.nan, math.nan
    n, _, sx, sy, sxx, syy, sxy, sdd = (float(v) for v in f0_sums)
    cov, vx, vy = sxy - sx * sy / n, sxx - sx * sx / n, syy - sy * sy / n
    corr = cov / math.sqrt(vx * vy) if vx > 0.0 and vy > 0.0 else math.nan
    return mcd, math.sqrt(sdd / n), corr


def format_mean(means, spkemb_sim=None):
    """The reference's closing line (evaluate.py:212-311): what the recipes grep for after "INFO: "."""
    parts = [f"MCD = {means['MCD']:.2f}", f"F0RMSE = {means['F0RMSE']:.3f}", f"F0CORR = {means['F0CORR']:.3f}", f"DDUR = {means['DDUR']:.3f}"] \
        if means is not None else []
    if spkemb_sim is not None:
        parts.append(f"SPKEMB SIM = {spkemb_sim:.3f}")
    return "Mean " + "; ".join(parts)


class Evaluator:
    """The stage on one device.  Extractors are kept per sampling rate, the pitch tables per f0 range (inside ``Pitch``).  The stage functions
    (``cepstra``, ``active_frames``, ``dtw``, ``path_stats``, ``trimmed_length``) are public: the tests pin them one at a time."""

    def __init__(self, device="cuda"):
        self.device = require_cuda(device, "jatts_amd.evaluate")
        self._fs = {}

    def front(self, fs):
        """-> (LogMelExtractor, the DCT as a prepared k = 1 conv, Pitch, the trim's Stft) of a sampling rate"""
        fs = int(fs)
        if fs not in self._fs:
            hop = int(round(fs * MCEP_SHIFT_MS / 1000.0))
            mel = LogMelExtractor(self.device, fs, fft_size=MCEP_FFTL, hop_size=hop, num_mels=N_MELS, fmin=MEL_FMIN, fmax=fs / 2.0, eps=1e-10,
                                  log_base=None)
            with hip.operands(None):      # exact f32 always
                dct = hip.PackedConv(torch.from_numpy(dct_matrix()), None, F32, self.device)
            pitch = Pitch(fs, n_fft=F0_FFT, hop_length=hop, use_token_averaged_f0=False, device=self.device)
            self._fs[fs] = (mel, dct, pitch, Stft(self.device, TRIM_FFT, TRIM_HOP))
        return self._fs[fs]

    def pack(self, waves):
        """numpy arrays, CPU tensors and device tensors, mixed -> one PackedWaves on the device; a PackedWaves is passed through"""
        if isinstance(waves, PackedWaves):
            return waves
        return PackedWaves.from_list([torch.as_tensor(w).reshape(-1).to(self.device, torch.float32) for w in waves], self.device)

    # ---- the stages
    @torch.no_grad()
    def cepstra(self, waves, fs):
        """-> (RaggedBatch over frames, cepstra f32 (rows, 40), pow_sum f32 (rows,), log-mel f32 (rows, 128))"""
        mel, dct, _, _ = self.front(fs)
        rb, mag, pow_sum = mel.stft.magnitude(self.pack(waves), want_pow=True)
        logmel = hip.logmel_post(mel.mel_w(rb, mag), mel.num_mels, mel.ld_out, mel.eps, mel.log_code)
        return rb, dct(rb, logmel), pow_sum, logmel

    def active_frames(self, rb, pow_sum, count=None):
        """-> (count int32 (n_seq,), idx int32 (rows,)): frames with npow > -20 dB, i.e. P_t > 10^-2 mean_t P_t"""
        require_device_tensor(pow_sum, "active_frames takes a device tensor")
        return hip.frame_select(rb, pow_sum, hip.SELECT_MEAN, 10.0 ** (VAD_DB / 10.0), count)

    def dtw(self, geo, a, b=None):
        """Distances and exact DTW of the pairs ``geo`` over rows of ``a`` (and ``b``, default the same matrix) -> hip.dtw's result"""
        require_device_tensor(a, "dtw takes device tensors")
        return hip.dtw(geo, hip.pairwise_dist(geo, a, a if b is None else b, MCEP_DIM + 1))

    def path_stats(self, geo, path, a=None, b=None, x=None, y=None, out=None):
        plen, pi, pj, _ = path
        return hip.dtw_path_stats(geo, plen, pi, pj, a, b, None if a is None else MCEP_DIM + 1, x, y, out)

    @torch.no_grad()
    def trimmed_length(self, waves, fs, count=None):
        """-> int32 (n_seq, 2) on the device: first and last frame of an Stft(2048, 512) within 60 dB of the wave's maximum power sum;
        ``trim_samples`` turns a row into the trimmed length."""
        pw = self.pack(waves)
        rb, _, pow_sum = self.front(fs)[3].magnitude(pw, want_pow=True)
        return hip.frame_select(rb, pow_sum, hip.SELECT_MAX, 10.0 ** (-TRIM_TOP_DB / 10.0), count)[0]

    @staticmethod
    def trim_samples(first, last, n_samples):
        return 0 if first < 0 else min(int(n_samples), (int(last) + 1) * TRIM_HOP) - int(first) * TRIM_HOP

    # ---- the batch
    @torch.no_grad()
    def evaluate_batch(self, items, fs, f0min, f0max, want_paths=False):
        """``items``: (generated wave x, ground-truth wave y[, sample id]) per pair, all at ``fs`` and of one f0 range -> one dict
        {"MCD", "F0RMSE", "F0CORR", "DDUR"} of Python floats per pair (with ``want_paths`` also "path": the power path as two int arrays).
        ValueError naming the sample when the VAD leaves a side without an active frame or a side exceeds the DTW's row cap."""
        B = len(items)
        if B == 0:
            return []
        names = [str(it[2]) if len(it) > 2 else f"pair {i}" for i, it in enumerate(items)]
        pw = self.pack([it[0] for it in items] + [it[1] for it in items])       # utterances 0 .. B-1: x, B .. 2B-1: y
        _, _, pitch, _ = self.front(fs)
        counts = torch.empty(8 * B, dtype=torch.int32, device=self.device)      # active | voiced | (first, last) of the trim
        rb, cep, pow_sum, _ = self.cepstra(pw, fs)
        _, idx_a = self.active_frames(rb, pow_sum, counts[:2 * B])
        rb_f, f0, _ = pitch.raw(pw, f0min, f0max)
        if rb_f.lens != rb.lens:
            raise AssertionError("evaluate: the pitch track and the cepstra disagree on the frame count")
        _, idx_v = hip.frame_select(rb, f0, hip.SELECT_POSITIVE, 0.0, counts[2 * B:4 * B])
        self.trimmed_length(pw, fs, counts[4 * B:])
        c = counts.cpu().numpy()                                                # read 1 of 2: sizes the DTW
        na, nv, trim = c[:2 * B].tolist(), c[2 * B:4 * B].tolist(), c[4 * B:].reshape(2 * B, 2)
        for p in range(B):
            if na[p] == 0 or na[B + p] == 0:
                raise ValueError(f"{names[p]}: no active frame in the {'generated' if na[p] == 0 else 'ground-truth'} wave (it is silent)")
        cap = hip.dtw_max_rows()
        for p in range(B):
            if na[p] > cap:
                raise ValueError(f"{names[p]}: {na[p]} active frames in the generated wave, the DTW takes at most {cap} rows")

        stats = torch.empty(2 * B, 8, dtype=torch.float64, device=self.device)
        rb_a = hip.RaggedBatch(na, self.device)
        act = hip.gather_rows(rb, idx_a, rb_a, cep)
        geo = hip.PairGeometry(na[:B], na[B:], rb_a.cu_host[:B], rb_a.cu_host[B:2 * B])
        path = self.dtw(geo, act)
        self.path_stats(geo, path, a=act, b=act, out=stats[:B])

        voiced = [p for p in range(B) if nv[p] > 0 and nv[B + p] > 0]
        if voiced:
            rb_v = hip.RaggedBatch(nv, self.device)
            vcep, vf0 = hip.gather_rows(rb, idx_v, rb_v, cep), hip.gather_rows(rb, idx_v, rb_v, f0)
            geo_v = hip.PairGeometry([nv[p] for p in voiced], [nv[B + p] for p in voiced], [rb_v.cu_host[p] for p in voiced],
                                     [rb_v.cu_host[B + p] for p in voiced])
            self.path_stats(geo_v, self.dtw(geo_v, vcep), x=vf0, y=vf0, out=stats[B:B + len(voiced)])
        s = stats.cpu().numpy()                                                 # read 2 of 2: the sums
        f0_row = {p: B + k for k, p in enumerate(voiced)}
        out = []
        for p in range(B):
            if p not in f0_row:
                log.warning(NO_F0_WARNING)
            mcd, rmse, corr = metrics_from_sums(s[p], s[f0_row[p]] if p in f0_row else None)
            lx = self.trim_samples(trim[p][0], trim[p][1], pw.lens[p])
            ly = self.trim_samples(trim[B + p][0], trim[B + p][1], pw.lens[B + p])
            out.append({"MCD": float(mcd), "F0RMSE": float(rmse), "F0CORR": float(corr), "DDUR": float(abs(lx - ly) / fs)})
        if want_paths:        # (tests and tools only: a third read)
            plen, pi, pj = path[0].cpu().numpy(), path[1].cpu().numpy(), path[2].cpu().numpy()
            for p in range(B):
                o = geo.p_off[p]
                out[p]["path"] = (pi[o:o + plen[p]].copy(), pj[o:o + plen[p]].copy())
        return out


_EVALUATORS = {}


def evaluator(device="cuda"):
    key = str(torch.device(device))
    if key not in _EVALUATORS:
        _EVALUATORS[key] = Evaluator(device)
    return _EVALUATORS[key]


def refuse_gv(calculate_gv):
    if calculate_gv:
        raise NotImplementedError("calculate_gv: the global variance is not computed by jatts_amd.evaluate (out of scope of stage 5 here)")


def calculate_mcd_f0(x, y, fs, f0min, f0max, calculate_gv=False):
    """The reference's signature (dtw_based.py:17) for one pair: ``x`` the generated wave, ``y`` the ground truth, both in [-1, 1] at ``fs``."""
    refuse_gv(calculate_gv)
    return evaluator().evaluate_batch([(x, y)], fs, f0min, f0max)[0]
