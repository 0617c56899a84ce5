"""CPU: the definition of the sample-rate converter (jatts_amd.features.resample_*) against the real scipy.signal.firwin /
resample_poly and tests/golden/resample_kat.npz, the seconds-to-samples rule of read_audio, the shared wav decoding, and the
preprocess CLI's refusals.  No compute calls (no GPU here).  Parity with librosa.load(sr=...) (soxr_hq) is NOT pinned anywhere."""
import csv
import importlib.util
import json
import os
import wave

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

RATIOS = [(48000, 24000), (48000, 16000), (24000, 16000), (44100, 24000), (22050, 24000), (24000, 44100), (24000, 48000)]
DESIGNS = [dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492), dict(zeros=10, rolloff=1.0, beta=5.0)]


@pytest.fixture(scope="module")
def kat():
    z = np.load(os.path.join(GOLDEN, "resample_kat.npz"))
    return z, json.loads(str(z["cases"]))


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_resample", os.path.join(GOLDEN, "make_golden_resample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("sr_in,sr_out", RATIOS)
@pytest.mark.parametrize("design", DESIGNS, ids=["kaiser_best", "scipy_default"])
def test_taps_equal_scipy_firwin(sr_in, sr_out, design):
    from scipy.signal import firwin

    from jatts_amd import features as F
    up, down = F.resample_ratio(sr_in, sr_out)
    assert up * sr_in == down * sr_out and np.gcd(up, down) == 1
    m = max(up, down)
    ref = up * firwin(2 * design["zeros"] * m + 1, design["rolloff"] / m, window=("kaiser", design["beta"]))
    h64 = F.resample_design(sr_in, sr_out, **design)
    assert h64.dtype == np.float64 and h64.shape == ref.shape
    assert (np.abs(h64 - ref) <= 1e-14 * np.abs(ref)).all()                        # element by element
    taps = F.resample_taps(sr_in, sr_out, **design)
    assert taps.dtype == np.float32 and np.array_equal(taps, h64.astype(np.float32))       # rounded once
    assert (np.abs(taps.astype(np.float64) - ref) <= (2.0 ** -24 + 1e-14) * np.abs(ref)).all()
    assert abs(float(h64.sum()) - up) <= 1e-12 * up                                 # unit DC gain per phase set


def test_default_design_is_kaiser_best():
    from jatts_amd import features as F
    assert (F.RESAMPLE_ZEROS, F.RESAMPLE_ROLLOFF, F.RESAMPLE_BETA) == (64, 0.9475937167399596, 14.769656459379492)
    assert np.array_equal(F.resample_taps(48000, 24000), F.resample_taps(48000, 24000, **DESIGNS[0]))
    assert F.resample_taps(48000, 24000).size == 2 * 64 * 2 + 1


def test_output_length_rule():
    from jatts_amd import features as F
    for up, down in [(1, 2), (1, 3), (2, 3), (80, 147), (160, 147), (147, 80), (2, 1)]:
        for n in (0, 1, 2, 3, 146, 147, 148, 4001, 240000):
            want = (n * up + down - 1) // down
            assert F.resample_out_len(n, up, down) == want == int(np.ceil(n * up / down))


def test_block_geometry_examples():
    """The three examples the kernel's design was sized on."""
    from jatts_amd import features as F
    g = F.resample_geometry(1, 2, 128)
    assert (g["r"], g["Nb"], g["Nbp"], g["K"], g["hop_b"], g["L"]) == (32, 32, 32, 320, 64, 128)
    g = F.resample_geometry(80, 147, 64 * 147)
    assert (g["r"], g["Nb"], g["Nbp"], g["K"], g["hop_b"], g["L"]) == (1, 80, 96, 384, 147, 117)
    g = F.resample_geometry(147, 80, 64 * 147)
    assert (g["r"], g["Nb"], g["Nbp"], g["K"], g["hop_b"], g["L"]) == (1, 147, 160, 256, 80, 64)


def test_table_times_framed_input_reproduces_resample_poly(kat):
    """Y = X W in float64 against the fixture's scipy answers to 1e-12: pins the block indexing, L, K and the column padding."""
    from jatts_amd import features as F
    z, cases = kat
    for c in cases:
        up, down = F.resample_ratio(c["sr_in"], c["sr_out"])
        assert (up, down) == (c["up"], c["down"])
        taps = F.resample_taps(c["sr_in"], c["sr_out"], c["zeros"], c["rolloff"], c["beta"])
        g = F.resample_geometry(up, down, taps.size // 2)
        w = F.resample_table(taps, up, down)
        assert w.dtype == np.float32 and w.shape == (g["K"], g["Nbp"]) and g["K"] % 64 == 0 and g["Nbp"] % 32 == 0
        assert not w[:, g["Nb"]:].any()                                             # padding columns are zero
        assert np.isin(w[w != 0], taps).all()                                       # pure indexing: every entry IS a tap
        assert sorted(w[w != 0].tolist()) == sorted(taps[taps != 0].tolist() * g["r"])        # ... and every tap is there, once per phase set
        for key in ("noise", "chirp"):
            x = z[f"x_{key}"].astype(np.float64)
            y64 = z[f"{c['name']}_{key}_y64"]
            n_out = F.resample_out_len(x.size, up, down)
            assert y64.shape == (n_out,)
            blocks = -(-n_out // g["Nb"])
            idx = np.arange(blocks)[:, None] * g["hop_b"] - g["L"] + np.arange(g["K"])[None, :]
            xq = np.where((idx >= 0) & (idx < x.size), x[np.clip(idx, 0, x.size - 1)], 0.0)
            y = (xq @ w.astype(np.float64))[:, :g["Nb"]].reshape(-1)[:n_out]
            assert np.abs(y - y64).max() <= 1e-12, (c["name"], key)


def test_refusals_name_the_limit():
    from jatts_amd import features as F
    with pytest.raises(ValueError, match=r"K <= 2048"):
        F.resample_table(F.resample_taps(48000, 1000), 1, 48)
    with pytest.raises(ValueError, match=r"Nbp <= 512"):
        F.resample_table(F.resample_taps(3, 1000), 1000, 3)
    # (a table larger than 4 MiB is refused as well; with K <= 2048 and Nbp <= 512 it has at most exactly 4 MiB)
    assert F.RESAMPLE_MAX_K * F.RESAMPLE_MAX_NBP * 4 == F.RESAMPLE_MAX_TABLE_BYTES
    with pytest.raises(ValueError):
        F.resample_taps(24000, 24000)
    with pytest.raises(ValueError):
        F.resample_ratio(44100.5, 24000)
    with pytest.raises(ValueError):
        F.resample_table(np.zeros(4, np.float32), 1, 2)
    # scipy's own default design stays reachable through the arguments
    assert F.resample_table(F.resample_taps(44100, 24000, zeros=10, rolloff=1.0, beta=5.0), 80, 147).shape == (192, 96)


def test_seconds_to_samples_truncates_at_the_native_rate():
    from jatts_amd import features as F
    assert F.seconds_to_samples(None, None, 48000) == (0, None)
    assert F.seconds_to_samples("0.1", None, 48000) == (0, None) and F.seconds_to_samples(None, 2.0, 48000) == (0, None)    # both or neither
    assert F.seconds_to_samples("0.05", "0.25", 48000) == (2400, int((0.25 - 0.05) * 48000))
    assert F.seconds_to_samples(0.0, 0.1234, 22050) == (0, 2720)                  # 2720.97: truncation, not rounding
    assert F.seconds_to_samples(0.1234, 0.5, 22050) == (2720, 8304)               # 2720.97 and 8304.03
    assert F.seconds_to_samples(1.00001, 1.5, 22050) == (22050, 11024)            # 22050.22 and 11024.78
    with pytest.raises(ValueError):
        F.seconds_to_samples(0.5, 0.25, 48000)


def test_wav_decoding_is_shared_and_unchanged(tmp_path):
    from jatts_amd.spkemb import load_wav
    from jatts_amd.wavio import decode_wav
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, size=(500, 2), dtype=np.int16)
    pcm[0] = (-32768, 32767)
    for ch, name in ((1, "mono.wav"), (2, "stereo.wav")):
        with wave.open(str(tmp_path / name), "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(2)
            w.setframerate(44100)
            w.writeframes(pcm[:, :ch].tobytes())
        a, rate = decode_wav(str(tmp_path / name))
        assert rate == 44100 and a.dtype == np.float32 and a.shape == (500, ch)
        assert np.array_equal(a, pcm[:, :ch].astype(np.float32) / 32768.0)
        t, rate = load_wav(str(tmp_path / name))                                    # the speaker front end keeps channel 0
        assert rate == 44100 and t.dim() == 1 and np.array_equal(t.numpy(), pcm[:, 0].astype(np.float32) / 32768.0)


@pytest.mark.parametrize("feat", ["pitch", "encodec", "encodec_48khz"])
def test_cli_refuses_missing_extractors_before_writing(tmp_path, feat):
    import yaml

    from jatts_amd.bin import preprocess
    conf = dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=1200, window="hann", num_mels=80, fmin=80, fmax=7600,
                global_gain_scale=1.0, feat_list=["mel", feat], pitch_extract_type="dio")
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(conf))
    rows = [{"sample_id": "a", "wav_path": str(tmp_path / "missing.wav")}]
    with open(tmp_path / "d.csv", "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0]))
        wr.writeheader()
        wr.writerows(rows)
    before = (tmp_path / "d.csv").read_bytes()
    with pytest.raises(NotImplementedError, match="pyworld" if feat == "pitch" else "encodec package"):
        preprocess.main(["--csv", str(tmp_path / "d.csv"), "--dumpdir", str(tmp_path / "dump"), "--config", str(tmp_path / "conf.yaml"),
                         "--f0_path", str(tmp_path / "f0.yaml"), "--verbose", "0"])
    assert not (tmp_path / "dump").exists() and (tmp_path / "d.csv").read_bytes() == before
    spk = dict(feat_list=["mel", "spkemb"], spkemb_extract_type="speechbrain")
    assert preprocess.check_feat_list(dict(spk, spkemb_checkpoint="embedding_model.ckpt")) == ["mel", "spkemb"]
    if not os.environ.get("JATTS_SPKEMB_CHECKPOINT"):
        with pytest.raises(RuntimeError, match="spkemb_checkpoint"):                # no randomly initialised embedding model
            preprocess.check_feat_list(spk)
    with pytest.raises(ValueError, match="Unsupported energy extractor type"):
        preprocess.check_feat_list(dict(feat_list=["mel", "energy"], energy_extract_type="other"))


def test_new_symbols_are_declared_with_their_citation():
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    from jatts_amd import _abi
    for name in ("jatts_resample", "jatts_wave_gain_peak"):
        assert name in _abi.PROTOTYPES and f"int {name}(" in hdr
    assert "utils/utils.py:201-234" in hdr and "#define JATTS_ABI_VERSION 8" in hdr
    assert "resample.hip" in open(os.path.join(ROOT, "jatts_amd", "csrc", "Makefile")).read()


def test_recipes_source_stage1_and_keep_stage4_the_default():
    import glob
    scripts = sorted(glob.glob(os.path.join(ROOT, "egs", "*", "tts*", "run.sh")))
    assert len(scripts) == 6
    for s in scripts:
        t = open(s).read()
        assert "egs/common/stage1.sh" in t and "stage1_features" in t and "\nstage=4 " in t and "\nstop_stage=4 " in t, s
    sh = open(os.path.join(ROOT, "egs", "common", "stage1.sh")).read()
    assert "jatts_amd.bin.preprocess" in sh and "jatts_amd.bin.compute_statistics" in sh and "stats.npz" in sh and "&\n" not in sh


def test_fixture_regenerates_byte_for_byte(tmp_path):
    gen = _generator()
    gen.main(str(tmp_path / "again.npz"))
    assert (tmp_path / "again.npz").read_bytes() == open(os.path.join(GOLDEN, "resample_kat.npz"), "rb").read()
    assert os.path.getsize(os.path.join(GOLDEN, "resample_kat.npz")) < 512 * 1024
