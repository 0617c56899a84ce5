"""CPU: the autocorrelation F0 estimator's definition holds up against ground truth in its float64 restatement
(tests/pitch_reference.py), the host-side table of jatts_acf_from_mag is the definition's, the geometry and the CLI refuse what they must,
and the new entry points are declared.  No GPU here; tests/test_pitch_gpu.py holds the kernels to the same restatement."""
import os
import re

import numpy as np
import pytest

import pitch_reference as PR
from conftest import ROOT

GEOMETRIES = [(24000, 2048, 300), (22050, 1024, 256), (16000, 1024, 160)]
SWEEPS = [(90, 140), (120, 300), (200, 380), (380, 200), (75, 110), (300, 395)]
F0MIN, F0MAX = 70, 400


def test_restatement_against_ground_truth():
    """Over three geometries and six sweeps of 1.2 s: no gross error (> 5 %), no fully voiced frame called unvoiced, no fully silent frame
    called voiced, fine error <= 3e-3 relative (2 x the worst observed, 1.4e-3: the frame-centre truth of a sweep is itself only that sharp)."""
    gross = miss = false_voiced = n_full = 0
    worst = 0.0
    for sr, n_fft, hop in GEOMETRIES:
        for i, (fa, fb) in enumerate(SWEEPS):
            x, f_true, on = PR.make_signal(sr, fa, fb, 1.2, seed=100 + i)
            res = PR.analyse(x, sr, n_fft, hop, F0MIN, F0MAX)
            truth, full, silent = PR.frame_truth(f_true, on, hop, res["W"])
            n_full += int(full.sum())
            miss += int((full & ~res["voiced"]).sum())
            false_voiced += int((silent & res["voiced"]).sum())
            ok = full & res["voiced"]
            rel = np.abs(res["f0"][ok] / truth[ok] - 1.0)
            gross += int((rel > 0.05).sum())
            if (rel <= 0.05).any():
                worst = max(worst, float(rel[rel <= 0.05].max()))
    print(f"fully voiced frames {n_full}, gross {gross}, misses {miss}, false voicings {false_voiced}, worst fine error {worst:.3e}")
    assert n_full > 1000
    assert gross == 0 and miss == 0 and false_voiced == 0
    assert worst <= 3e-3


def test_restatement_post_equals_the_reference(golden_dir):
    """tests/pitch_reference.post (what the end-to-end GPU test chains behind the restatement) against the real Dio.forward."""
    z = np.load(os.path.join(golden_dir, "pitch_post_kat.npz"))
    for i in range(int(z["n"])):
        fl = int(z[f"feat_length_{i}"])
        for cont in (1, 0):
            for log in (1, 0):
                got = PR.post(z[f"track_{i}"], None if fl < 0 else fl, z[f"durations_{i}"], bool(cont), bool(log))
                np.testing.assert_allclose(got, z[f"out_{i}_{cont}{log}"], rtol=1e-13, atol=0)
                got = PR.post(z[f"track_{i}"], None if fl < 0 else fl, None, bool(cont), bool(log))
                np.testing.assert_allclose(got, z[f"frames_{i}_{cont}{log}"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("sr,n_fft,f0min,f0max", [(24000, 2048, 40, 400), (24000, 2048, 70, 400), (22050, 1024, 70, 400), (16000, 512, 110, 500)])
def test_acf_table_is_the_definition(sr, n_fft, f0min, f0max):
    """sum_k P[k] table[k][tau] against float64 irfft(P) * rw(0) / rw(tau) on random power spectra: 1e-6 relative to r(0), the single f32
    rounding of the table's entries (2^-24 per entry, |entry| <= c_k / n_fft * rw(0) / rw(tau))."""
    from jatts_amd import features
    lo, hi, w_len = features.pitch_geometry(sr, n_fft, f0min, f0max)
    assert (lo, hi, w_len) == PR.geometry(sr, n_fft, f0min, f0max)
    win = features.padded_window("hann", w_len, n_fft)
    np.testing.assert_allclose(win, PR.hann_padded(w_len, n_fft), atol=1e-15)
    table = features.acf_table(win, n_fft, hi)
    n_bins = n_fft // 2 + 1
    assert table.dtype == np.float32 and table.shape == ((n_bins + 63) // 64 * 64, (hi + 2 + 31) // 32 * 32)
    assert not table[n_bins:].any() and not table[:, hi + 2:].any()
    g = np.random.default_rng(5)
    p = g.random((6, n_bins)) ** 4
    got = p @ table[:n_bins, :hi + 2].astype(np.float64)
    rw = np.fft.irfft(np.abs(np.fft.rfft(win)) ** 2, n=n_fft)[:hi + 2]
    want = np.fft.irfft(p, n=n_fft, axis=1)[:, :hi + 2] * (rw[0] / rw)[None, :]
    err = np.abs(got - want).max(axis=1) / want[:, 0]
    print("acf_table: worst error relative to r(0)", err.max())
    assert err.max() <= 1e-6


def test_geometry_examples_and_refusals():
    from jatts_amd import features
    assert features.pitch_geometry(24000, 2048, 40, 400)[2] == 1446
    assert features.pitch_geometry(24000, 2048, 70, 400)[2] == 1026
    with pytest.raises(ValueError, match="raise f0min or fft_size"):
        features.pitch_geometry(24000, 1024, 40, 400)          # hi = 600: W = 422 < 2 hi
    with pytest.raises(ValueError, match="raise f0min or fft_size"):
        features.pitch_geometry(24000, 2048, 30, 400)          # hi = 800: W = 1246 < 1600
    assert features.pitch_geometry(1000, 256, 100, 500) == (2, 10, 30)      # lo = 2 is the least
    with pytest.raises(ValueError, match="raise f0min or fft_size"):
        features.pitch_geometry(1000, 256, 100, 1000)          # lo = 1, with a window (30 >= 20) that would do
    with pytest.raises(ValueError):
        features.pitch_geometry(24000, 2048, 400, 70)


def test_check_feat_list_accepts_acf_and_refuses_the_rest(caplog):
    from jatts_amd.bin import preprocess
    base = {"feat_list": ["mel", "pitch"], "pitch_extract_type": "acf"}
    with caplog.at_level("WARNING"):
        assert preprocess.check_feat_list(base) == ["mel", "pitch"]
    assert any("UNPINNED" in r.getMessage() or "unpinned" in r.getMessage() for r in caplog.records)
    with pytest.raises(NotImplementedError, match="pyworld"):
        preprocess.check_feat_list({**base, "pitch_extract_type": "dio"})
    with pytest.raises(NotImplementedError, match="pyworld"):
        preprocess.check_feat_list({"feat_list": ["mel", "pitch"]})
    with pytest.raises(ValueError, match="Unsupported pitch extractor type: harvest"):
        preprocess.check_feat_list({**base, "pitch_extract_type": "harvest"})
    assert preprocess.check_feat_list({"feat_list": ["mel"], "pitch_extract_type": "acf"}) == ["mel"]


def test_new_symbols_are_declared_with_their_citation(lib):
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    for name in ("jatts_acf_from_mag", "jatts_pitch_pick", "jatts_f0_continuous_log"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name)
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, hdr, re.S)
        assert m and re.search(r"dio\.py:\d+", m.group(1)), name
    assert "UNPINNED" in hdr[hdr.index("Stage-1 pitch"):hdr.index("jatts_acf_from_mag(")]
    assert _abi.ABI_VERSION == 8 and lib.jatts_abi_version() == 8
    assert "pitch.hip" in open(os.path.join(ROOT, "jatts_amd", "csrc", "Makefile")).read()
