"""GPU: ``python -m jatts_amd.bin.preprocess`` (stage 1 of the recipes) on four toy 48 kHz PCM16 files, then
``jatts_amd.bin.compute_statistics`` on its dumps, then the whole stage through ``egs/jsut/tts2/run.sh --stage 1 --stop_stage 1``.

The dumps are compared bit for bit with the host interface (``features.resample`` of the decoded file, ``logmelfilterbank`` of the
dumped wave): the CLI's batching changes no bits.  The numbers themselves are pinned in tests/test_resample_gpu.py and
tests/test_features_gpu.py."""
import csv
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONF = dict(sampling_rate=24000, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=80, fmax=7600,
            global_gain_scale=2.0, feat_list=["mel"], log_base=10.0)
SR_NATIVE = 48000


def _write_toy_data(d, names=("utt0", "utt1", "utt2", "loud")):
    """Four files of about 0.3 s; ``loud`` peaks at 0.8 (clips under the gain of 2), the others at 0.3.  utt1 is cut by start / end."""
    rng = np.random.default_rng(7)
    rows = []
    for i, name in enumerate(names):
        n = 14000 + 331 * i
        t = np.arange(n) / SR_NATIVE
        amp = 0.8 if name == "loud" else 0.3
        x = amp * np.sin(2 * np.pi * (180.0 + 40.0 * i) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 1e-3 * rng.standard_normal(n)
        x = np.clip(x, -amp, amp)
        path = d / f"{name}.wav"
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(SR_NATIVE)
            w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        rows.append({"sample_id": name, "wav_path": str(path), "start": "0.0213" if name == "utt1" else "",
                     "end": "0.2701" if name == "utt1" else "", "phonemes": "a b"})
    return rows


def _write_csv(path, rows):
    with open(path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0]))
        wr.writeheader()
        wr.writerows(rows)


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return env


def _check_dumps(feats_dir, csv_path, rows, cuda):
    from jatts_amd import features as F
    from jatts_amd.wavio import decode_wav
    with open(csv_path, newline="") as f:
        out = list(csv.DictReader(f))
    assert [r["sample_id"] for r in out] == [r["sample_id"] for r in rows if r["sample_id"] != "loud"]       # the clipping one is gone
    assert not os.path.exists(os.path.join(feats_dir, "loud.npz"))
    for r in out:
        assert r["feat_path"] == os.path.realpath(os.path.join(feats_dir, r["sample_id"] + ".npz")) and r["phonemes"] == "a b"
        with np.load(r["feat_path"]) as z:
            assert sorted(z.files) == ["mel", "wave"]
            wav, mel = z["wave"], z["mel"]
        a, rate = decode_wav(r["wav_path"])
        assert rate == SR_NATIVE
        a = a[:, 0]
        if r["start"]:
            first, count = F.seconds_to_samples(r["start"], r["end"], rate)
            assert (first, count) == (1022, 11942)
            a = a[first:first + count]
        want = F.resample(torch.from_numpy(a.copy()).to(cuda), rate, CONF["sampling_rate"]) * np.float32(CONF["global_gain_scale"])
        assert wav.dtype == np.float32 and wav.shape == (-(-a.size // 2),)
        assert np.array_equal(wav.view(np.uint32), want.cpu().numpy().view(np.uint32))
        want_mel = F.logmelfilterbank(wav, **{k: v for k, v in CONF.items() if k not in ("global_gain_scale", "feat_list")})
        assert mel.dtype == np.float32 and mel.shape == (1 + wav.size // CONF["hop_size"], 80)
        assert np.array_equal(mel.view(np.uint32), want_mel.view(np.uint32))
    return out


def test_preprocess_cli_then_compute_statistics(cuda, lib, tmp_path):
    rows = _write_toy_data(tmp_path)
    _write_csv(tmp_path / "train.csv", rows)
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(CONF))
    feats = tmp_path / "dump" / "feats"
    r = subprocess.run([sys.executable, "-m", "jatts_amd.bin.preprocess", "--csv", str(tmp_path / "train.csv"), "--dumpdir", str(feats),
                        "--config", str(tmp_path / "conf.yaml"), "--f0_path", str(tmp_path / "no_f0.yaml"), "--batch-size", "3",
                        "--verbose", "1"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{tmp_path / 'loud.wav'} causes clipping (max: " in r.stderr and "it is better to re-consider global gain scale." in r.stderr
    assert f"{tmp_path / 'loud.wav'} returns None. Skip." in r.stderr
    out = _check_dumps(str(feats), tmp_path / "train.csv", rows, cuda)
    r = subprocess.run([sys.executable, "-m", "jatts_amd.bin.compute_statistics", "--csv", str(tmp_path / "train.csv"), "--out",
                        str(tmp_path / "stats.npz"), "--verbose", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(tmp_path / "stats.npz") as z:
        assert sorted(z.files) == ["mel_mean", "mel_scale"] and z["mel_mean"].shape == (80,) and z["mel_scale"].dtype == np.float32
        allmel = np.concatenate([np.load(o["feat_path"])["mel"] for o in out]).astype(np.float64)
        assert np.allclose(z["mel_mean"], allmel.mean(axis=0), rtol=1e-5, atol=1e-5) and (z["mel_scale"] > 0).all()


def test_energy_and_spkemb_dumps_equal_the_host_interface(cuda, lib, tmp_path):
    """feat_list mel + energy + spkemb, in this process: token-averaged energy through features.Energy (the csv carries durations, whose
    sum the mel length is asserted against, preprocess.py:258-261), the speaker embedding through SpkEmbExtractor from the configured
    checkpoint; a wrong duration sum is refused in the reference's words."""
    from jatts_amd import features as F
    from jatts_amd.bin import preprocess
    from jatts_amd.spkemb import ECAPA_TDNN, SpkEmbExtractor
    from jatts_amd.synthetic import synth_state_dict
    rows = _write_toy_data(tmp_path, names=("utt0", "utt1", "utt2"))
    frames = {}
    for r in rows:
        with wave.open(r["wav_path"]) as w:
            n = w.getnframes()
        n = 11942 if r["start"] else n
        frames[r["sample_id"]] = 1 + (-(-n // 2)) // CONF["hop_size"]
        r["durations"] = f"3 0 {frames[r['sample_id']] - 3}"
    ecfg = dict(channels=[256, 256, 256, 256, 768], attention_channels=64, se_channels=64, lin_neurons=192, res2net_scale=4)
    torch.save(synth_state_dict(ECAPA_TDNN(**ecfg).state_dict(), 5), tmp_path / "ecapa.ckpt")
    conf = dict(CONF, global_gain_scale=1.0, feat_list=["mel", "energy", "spkemb"], energy_extract_type="energy", spkemb_extract_type="speechbrain",
                spkemb_checkpoint=str(tmp_path / "ecapa.ckpt"), spkemb_params=ecfg, model_params={"reduction_factor": 1})
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(conf))
    _write_csv(tmp_path / "train.csv", rows)
    preprocess.main(["--csv", str(tmp_path / "train.csv"), "--dumpdir", str(tmp_path / "feats"), "--config", str(tmp_path / "conf.yaml"),
                     "--batch-size", "2", "--verbose", "0"])
    en = F.Energy(fs=24000, n_fft=CONF["fft_size"], win_length=None, hop_length=CONF["hop_size"], window="hann", reduction_factor=1, device=cuda)
    spk = SpkEmbExtractor(cuda, checkpoint=str(tmp_path / "ecapa.ckpt"), **ecfg)
    with open(tmp_path / "train.csv", newline="") as f:
        out = list(csv.DictReader(f))
    assert [o["sample_id"] for o in out] == ["utt0", "utt1", "utt2"]
    for o in out:
        with np.load(o["feat_path"]) as z:
            assert sorted(z.files) == ["energy", "mel", "spkemb", "wave"]
            d = [int(v) for v in o["durations"].split(" ")]
            assert z["mel"].shape == (sum(d), 80) and z["energy"].shape == (3,) and z["energy"].dtype == np.float32
            want = en.forward(z["wave"], feat_length=sum(d), durations=np.array(d))
            assert np.array_equal(z["energy"].view(np.uint32), want.view(np.uint32)) and z["energy"][1] == 0.0 and z["energy"][0] > 0.0
            assert z["spkemb"].shape == (192,) and z["spkemb"].dtype == np.float32
            assert np.allclose(z["spkemb"], spk.forward(o["wav_path"]), rtol=1e-4, atol=1e-6)      # (the CLI embeds a batch at a time)
    rows[0]["durations"] = "1 1 1"
    _write_csv(tmp_path / "bad.csv", rows[:1])
    with pytest.raises(AssertionError, match=r"utt0: mel duration \d+ and phoneme durations 3 don't match"):
        preprocess.main(["--csv", str(tmp_path / "bad.csv"), "--dumpdir", str(tmp_path / "bad"), "--config", str(tmp_path / "conf.yaml"), "--verbose", "0"])
    assert not os.path.exists(tmp_path / "bad" / "utt0.npz")


def test_recipe_run_sh_stage1(cuda, lib, tmp_path):
    """egs/jsut/tts2/run.sh --stage 1 --stop_stage 1: the reference's layout (dump/<set>/feats, data/<set>_raw_feat.csv,
    dump/train/stats.npz) from data/<set>.csv; data/<set>.csv itself is left as it was."""
    work = tmp_path / "recipe"
    os.makedirs(work / "data")
    os.makedirs(work / "conf")
    os.makedirs(work / "wav")
    rows = _write_toy_data(work / "wav")
    sets = {"train": rows, "dev": rows[:2], "test": rows[2:3]}
    for name, rs in sets.items():
        _write_csv(work / "data" / f"{name}.csv", rs)
    (work / "conf" / "toy.yaml").write_text(yaml.safe_dump(CONF))
    before = (work / "data" / "train.csv").read_bytes()
    r = subprocess.run(["bash", os.path.join(ROOT, "egs", "jsut", "tts2", "run.sh"), "--stage", "1", "--stop_stage", "1", "--conf",
                        "conf/toy.yaml", "--verbose", "1", "--preprocess_batch_size", "4"], cwd=work, env=dict(os.environ, PYTHON=sys.executable),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Stage 1: Feature extraction" in r.stdout and "Stage 4" not in r.stdout
    assert (work / "data" / "train.csv").read_bytes() == before
    for name, rs in sets.items():
        assert (work / "dump" / name / "preprocessing.log").exists()
        _check_dumps(str(work / "dump" / name / "feats"), work / "data" / f"{name}_raw_feat.csv", rs, cuda)
    assert (work / "dump" / "train" / "compute_statistics.log").exists()
    with np.load(work / "dump" / "train" / "stats.npz") as z:
        assert sorted(z.files) == ["mel_mean", "mel_scale"] and z["mel_mean"].shape == (80,)
    # a FastSpeech2-style config gets the CLI's refusal, not a silent skip; nothing goes on after the failing step
    (work / "conf" / "fs2.yaml").write_text(yaml.safe_dump(dict(CONF, feat_list=["mel", "pitch", "energy"], pitch_extract_type="dio")))
    r = subprocess.run(["bash", os.path.join(ROOT, "egs", "jsut", "tts2", "run.sh"), "--stage", "1", "--stop_stage", "1", "--conf",
                        "conf/fs2.yaml", "--dumpdir", "dump_fs2"], cwd=work, env=dict(os.environ, PYTHON=sys.executable),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "pyworld" in r.stdout + r.stderr
    assert not (work / "dump_fs2" / "train" / "stats.npz").exists() and not (work / "dump_fs2" / "dev").exists()
