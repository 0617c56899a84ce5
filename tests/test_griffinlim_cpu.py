"""CPU: the host side of Griffin-Lim -- the ISTFT table and envelope against ``torch.istft`` in float64, the mel
pseudo-inverse, the constructor's and the CLIs' refusals, the trainer's fallback rule and the ABI declarations."""
import logging
import os
import re

import numpy as np
import pytest
import torch

import griffinlim_reference as ref
from conftest import ROOT

GEOMS = [(256, 64, 256), (128, 50, 100), (1024, 300, 1024)]


def span_istft(X, w, n_fft, hop, table=None):
    """The package's ISTFT in float64 numpy, in the span form the kernel contracts: X complex (T, n_bins) -> ((T - 1) * hop,)."""
    from jatts_amd.vocoder import griffin_lim as g
    T, n_bins = X.shape
    nbp, J = (n_bins + 31) // 32 * 32, g.overlap(n_fft, hop)
    tab = g.istft_table(w, n_fft, hop, dtype=np.float64) if table is None else table
    flat = np.zeros((T + 2 * J, 2 * nbp))                     # J zero rows on either side: frames that do not exist
    flat[J:J + T, :n_bins], flat[J:J + T, nbp:nbp + n_bins] = X.real, X.imag
    flat = flat.reshape(-1)
    a, b, r = g.envelope_index(T, n_fft, hop)
    m = (np.arange((T - 1) * hop) + n_fft // 2) // hop
    env = g.envelope_sums(w, n_fft, hop)[a, b, r]
    K = J * 2 * nbp
    num = np.empty((T - 1) * hop)
    for mm in np.unique(m):                                    # output row mm contracts the rows mm - J + 1 .. mm of Xflat: ONE span
        sel = m == mm
        start = (mm - J + 1 + J) * 2 * nbp
        num[sel] = flat[start:start + K] @ tab[:, r[sel]]
    return num / env


@pytest.mark.parametrize("n_fft,hop,win", GEOMS)
def test_istft_table_and_envelope_equal_torch_istft(n_fft, hop, win):
    from jatts_amd.features.stft import padded_window
    w = padded_window("hann", win, n_fft)
    assert np.abs(w - ref.hann_padded(win, n_fft).numpy()).max() < 1e-15
    wt = torch.from_numpy(w)
    g = torch.Generator().manual_seed(n_fft + hop)
    for T in (2, 3, 9, 24):                                    # shorter than, around and beyond the overlap J
        X = torch.randn(T, n_fft // 2 + 1, generator=g, dtype=torch.complex128)
        want = ref.istft(X, wt, n_fft, hop).numpy()
        got = span_istft(X.numpy(), w, n_fft, hop)
        assert np.abs(got - want).max() <= 1e-12, (T, np.abs(got - want).max())
    x = ref.signal(23 * hop, 5)                                # the round trip: ISTFT(STFT(x)) = x
    C = ref.stft(x, wt, n_fft, hop)
    assert C.shape[0] == 24
    assert np.abs(span_istft(C.numpy(), w, n_fft, hop) - x.numpy()).max() <= 1e-12


def test_f32_tables_are_the_float64_ones_rounded_once():
    from jatts_amd.features.stft import padded_window
    from jatts_amd.vocoder import griffin_lim as g
    w = padded_window("hann", 100, 128)
    t64, t32 = g.istft_table(w, 128, 50, dtype=np.float64), g.istft_table(w, 128, 50)
    assert t32.dtype == np.float32 and t32.shape == (3 * 2 * 96, 64) and np.array_equal(t32, t64.astype(np.float32))
    assert not t32[:, 50:].any() and not t32.reshape(3, 2, 96, 64)[:, :, 65:].any()          # padding columns and bins
    e, r = g.envelope_sums(w, 128, 50), g.istft_envelope(w, 128, 50)
    assert r.shape == (3, 3, 64) and not r[:, :, 50:].any()
    ok = e >= g.NOLA_FLOOR
    assert np.array_equal(r[:, :, :50][ok], (1.0 / e[ok]).astype(np.float32)) and not r[:, :, :50][~ok].any()


def test_mel_pseudo_inverse():
    from jatts_amd.features.stft import mel_filterbank
    from jatts_amd.vocoder.griffin_lim import mel_pinv
    for fs, n_fft, n_mels, fmin, fmax in ((24000, 2048, 80, 80, 7600), (16000, 256, 20, None, None)):
        B = mel_filterbank(fs, n_fft, n_mels, fmin, fmax).T                      # (n_mels, n_bins)
        P = np.linalg.pinv(B)
        assert np.abs(P @ B @ P - P).max() <= 1e-10
        assert np.array_equal(mel_pinv(fs, n_fft, n_mels, fmin, fmax), P.astype(np.float32))
        rng = np.random.default_rng(0)
        c, mean, scale = rng.standard_normal((5, n_mels)), rng.standard_normal(n_mels) - 3.0, 0.5 + rng.random(n_mels)
        lin = ref.mel_to_linear(c, mean, scale, B, 10.0)
        assert lin.shape == (5, n_fft // 2 + 1) and lin.min() >= 1e-10


def test_constructor_refusals():
    from jatts_amd.vocoder import GriffinLim
    with pytest.raises(ValueError, match="hop_size larger than win_length"):
        GriffinLim("cuda", 128, 101, win_length=100)
    with pytest.raises(ValueError, match="momentum"):
        GriffinLim("cuda", 256, 64, momentum=1.0)
    with pytest.raises(ValueError, match="n_iter"):
        GriffinLim("cuda", 256, 64, n_iter=-1)
    with pytest.raises(ValueError, match="fft_size"):
        GriffinLim("cuda", 100, 25)
    with pytest.raises(ValueError, match="overlapping"):
        GriffinLim("cuda", 2048, 16)
    with pytest.raises(ValueError, match="hann"):
        GriffinLim("cuda", 256, 64, window="hamming")


def test_missing_config_key_is_named():
    from jatts_amd.vocoder import Spectrogram2Waveform
    from jatts_amd.vocoder.griffin_lim import CONFIG_KEYS
    full = {"fft_size": 256, "hop_size": 64, "sampling_rate": 16000, "num_mels": 20, "fmin": None, "fmax": None}
    assert set(CONFIG_KEYS) == set(full)
    stats = {"mean": np.zeros(20, np.float32), "scale": np.ones(20, np.float32)}
    for k in full:
        cfg = {kk: v for kk, v in full.items() if kk != k}
        with pytest.raises(ValueError, match=f"'{k}'"):
            Spectrogram2Waveform.from_config(cfg, stats, "cuda")


def test_trainer_without_the_stft_keys_keeps_the_skip(caplog):
    from jatts_amd import training

    def no_stats():
        raise AssertionError("the statistics are read only where the fallback is built")

    with caplog.at_level(logging.INFO):
        voc = training.griffin_lim_fallback({"model_type": "FastSpeech2", "fft_size": 256, "hop_size": 64}, no_stats, "cuda")
    assert voc is None
    assert [r.getMessage() for r in caplog.records] == ["No vocoder in the config: intermediate waveforms are skipped (no Griffin-Lim fallback)."]
    assert "griffin_lim_iters" not in training.unread_keys({"griffin_lim_iters": 4, "fft_size": 256})


def test_symbols_are_declared_in_the_header_and_the_prototypes():
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    for name, n_args in (("jatts_gl_stft_project", 13), ("jatts_gl_istft", 13), ("jatts_gl_exp", 10), ("jatts_gl_floor", 8), ("jatts_gl_init", 8)):
        m = re.search(r"\bint %s\(([^;]*?)\);" % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_abi.PROTOTYPES[name][1]), name
    assert _abi.ABI_VERSION == 8                  # additive: no bump
