"""CPU: the host side of jatts_amd.features -- mel matrix, window, framing geometry, DFT table, argument checks.

What is pinned: the mel matrix on transformers.audio_utils.mel_filter_bank(norm="slaney", mel_scale="slaney") (stored in
tests/golden/logmel_kat.npz by tests/golden/make_golden_logmel.py), the window on scipy, the framing on numpy.pad(mode="reflect").
What is NOT pinned: librosa itself (absent from the build environment)."""
import os

import numpy as np
import pytest
import scipy.signal
import torch

from jatts_amd import _abi, features

SETTINGS = {
    "a": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=2048, fmin=80, fmax=7600),
    "b": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=1200, fmin=80, fmax=7600),
    "c": dict(sampling_rate=22050, fft_size=1024, hop_size=256, win_length=None, fmin=None, fmax=None),
}


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_kat.npz"))


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_mel_filterbank_equals_the_fixture(kat, name):
    s = SETTINGS[name]
    m = features.mel_filterbank(s["sampling_rate"], s["fft_size"], 80, s["fmin"], s["fmax"])
    ref = kat[f"{name}_melmat"]
    assert m.dtype == np.float64 and m.shape == ref.shape == (s["fft_size"] // 2 + 1, 80)
    assert float(np.abs(m - ref).max()) <= 1e-12


@pytest.mark.parametrize("win,n_fft", [(2048, 2048), (1200, 2048), (None, 1024), (1023, 1024), (2, 64)])
def test_padded_window_is_scipy_hann_centred(win, n_fft):
    w = features.padded_window("hann", win, n_fft)
    wl = n_fft if win is None else win
    ref = np.zeros(n_fft)
    left = (n_fft - wl) // 2
    ref[left:left + wl] = scipy.signal.get_window("hann", wl, fftbins=True)
    assert w.dtype == np.float64 and np.array_equal(w, ref)


@pytest.mark.parametrize("n_fft,hop", [(2048, 300), (1024, 256), (64, 64)])
def test_framing_equals_numpy_reflect(n_fft, hop):
    rng = np.random.default_rng(0)
    for L in (n_fft // 2 + 1, 7 * hop, 20000):
        if L <= n_fft // 2:
            continue
        x = rng.standard_normal(L)
        xp = np.pad(x, n_fft // 2, mode="reflect")
        T = 1 + L // hop
        ref = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)])
        assert features.frame_count(L, n_fft, hop) == T
        idx = features.frame_indices(L, n_fft, hop)
        assert idx.shape == (T, n_fft) and idx.min() >= 0 and idx.max() < L
        assert np.array_equal(x[idx], ref)
    assert np.array_equal(features.reflect_index(np.array([-3, -1, 0, 4, 5, 7]), 5), [3, 1, 0, 4, 3, 1])


@pytest.mark.parametrize("win,n_fft", [(2048, 2048), (1200, 2048), (None, 1024)])
def test_dft_table_is_the_window_folded_in_float64(win, n_fft):
    w = features.padded_window("hann", win, n_fft)
    t = features.dft_table(w, n_fft)
    nb = n_fft // 2 + 1
    nbp = (nb + 31) // 32 * 32
    assert t.dtype == np.float32 and t.shape == (n_fft, 2 * nbp)
    n, k = np.arange(n_fft, dtype=np.int64)[:, None], np.arange(nb, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % n_fft).astype(np.float64) / n_fft          # angle reduced in integers: exact argument
    assert np.array_equal(t[:, :nb], (w[:, None] * np.cos(ang)).astype(np.float32))
    assert np.array_equal(t[:, nbp:nbp + nb], (-w[:, None] * np.sin(ang)).astype(np.float32))
    assert not t[:, nb:nbp].any() and not t[:, nbp + nb:].any()
    # and against the unreduced angle (float64 argument error ~ 1e-9 at n k ~ 2e6): within an f32 rounding of values <= 1
    raw = 2.0 * np.pi * (n * k).astype(np.float64) / n_fft
    assert float(np.abs(t[:, :nb] - w[:, None] * np.cos(raw)).max()) <= 2.0 ** -24
    assert float(np.abs(t[:, nbp:nbp + nb] + w[:, None] * np.sin(raw)).max()) <= 2.0 ** -24


def test_value_errors():
    with pytest.raises(ValueError, match="3.0 is not supported."):
        features.LogMelExtractor("cpu", 24000, log_base=3.0)
    with pytest.raises(ValueError, match="3.0 is not supported."):
        features.logmelfilterbank(np.zeros(4000, dtype=np.float32), 24000, log_base=3.0)
    with pytest.raises(ValueError):
        features.padded_window("hamming", None, 1024)
    with pytest.raises(ValueError):
        features.LogMelExtractor("cpu", 24000, window="blackman")
    with pytest.raises(ValueError):
        features.padded_window("hann", 2049, 2048)
    with pytest.raises(ValueError):
        features.LogMelExtractor("cpu", 24000, fft_size=4096)
    with pytest.raises(ValueError):
        features.LogMelExtractor("cpu", 24000, fft_size=1000)
    with pytest.raises(ValueError):
        features.LogMelExtractor("cpu", 24000, hop_size=0)
    with pytest.raises(ValueError):
        features.Energy(reduction_factor=2)
    with pytest.raises(ValueError):
        features.Energy(use_token_averaged_energy=True, reduction_factor=None)


def test_short_utterance_raises():
    with pytest.raises(ValueError):
        features.frame_count(1024, 2048, 300)
    with pytest.raises(ValueError):
        features.frame_indices(512, 1024, 256)
    assert features.frame_count(1025, 2048, 300) == 4


def test_cpu_device_raises_jatts_hip_error(lib):
    with pytest.raises(_abi.JattsHipError):
        features.LogMelExtractor("cpu", 24000, fft_size=2048, hop_size=300)
    with pytest.raises(_abi.JattsHipError):
        features.LogMelExtractor(torch.device("cpu"), 22050)
    with pytest.raises(_abi.JattsHipError):
        features.Energy(reduction_factor=1, device="cpu")
    from jatts_amd import hip
    with pytest.raises(_abi.JattsHipError):     # a CPU tensor at the wrapper
        hip.stft_mag(hip.RaggedBatch([4], "cpu"), torch.tensor([0, 1025], dtype=torch.int32), [1025], torch.zeros(1025),
                     torch.zeros(2048, 2 * 1056), 2048, 300, 1088)


# ---- the shared token-average path (features/common.py)
def test_token_spans_at_reduction_factor_1_wants_the_exact_sum():
    assert features.token_spans([[3, 0, 4]], [7], 1) == ([3], [3, 3, 7])
    for n in (6, 8):                                                          # the sum is off by +1 / -1
        with pytest.raises(ValueError, match=f"durations sum to 7, the utterance has {n} frames"):
            features.token_spans([[3, 0, 4]], [n], 1)


def test_token_spans_at_reduction_factor_2_allows_a_remainder_below_it():
    for n in (14, 15):                                                        # remainders 0 and 1
        assert features.token_spans([[3, 0, 4]], [n], 2) == ([3], [6, 6, 14])
    for n in (16, 13):                                                        # remainder 2, remainder -1
        with pytest.raises(ValueError, match=f"durations sum to 14, the utterance has {n} frames"):
            features.token_spans([[3, 0, 4]], [n], 2)


def test_token_spans_refusals_and_layout():
    with pytest.raises(ValueError, match="durations sum to"):
        features.token_spans([[5, -1, 3]], [7])                               # a negative duration, although the sum fits
    with pytest.raises(ValueError, match="one sequence per utterance"):
        features.token_spans([[7]], [7, 7])
    rng = np.random.default_rng(0)
    durs = [rng.integers(0, 5, size=n) for n in (1, 9, 4)] + [np.zeros(0, dtype=np.int64)]
    for rf, extra in ((1, [0, 0, 0, 0]), (3, [2, 0, 1, 0])):
        lens = [int(d.sum()) * rf + e for d, e in zip(durs, extra)]
        token_lens, cum = features.token_spans([torch.from_numpy(durs[0]), durs[1].tolist(), durs[2], durs[3]], lens, rf)
        assert token_lens == [d.size for d in durs]
        assert cum == np.concatenate([np.cumsum(d * rf) for d in durs]).tolist() and all(type(v) is int for v in cum)


def test_every_stage1_name_resolves_on_the_package():
    names = """LogMelExtractor logmelfilterbank Energy mel_filterbank padded_window dft_table frame_count frame_indices reflect_index
        FeatureStatistics STATS_ROWS_PER_GROUP stats_from_state save_stats standardize PackedWaves Resampler resample resample_ratio
        resample_taps resample_design resample_out_len resample_geometry resample_table RESAMPLE_ZEROS RESAMPLE_ROLLOFF RESAMPLE_BETA
        RESAMPLE_MAX_K RESAMPLE_MAX_NBP RESAMPLE_MAX_TABLE_BYTES seconds_to_samples read_audio read_audio_batch Pitch pitch_geometry
        window_autocorrelation acf_table PITCH_VOICING_THRESHOLD PITCH_SILENCE_THRESHOLD PITCH_OCTAVE_COST Stft token_spans""".split()
    assert [n for n in names if not hasattr(features, n)] == []
