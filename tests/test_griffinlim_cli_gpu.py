"""GPU: the two CLIs on a config WITHOUT a ``vocoder:`` entry -- stage 4 writes one wav per utterance through Griffin-Lim, stage 3 writes the
intermediate waveforms through it."""
import os
import wave

import numpy as np
import pytest
import torch
import yaml

from test_cli import _make_expdir
from test_train_cli_gpu import cli, corpora, fs2_config

pytestmark = pytest.mark.gpu

STFT_KEYS = {"fft_size": 1024, "hop_size": 256, "sampling_rate": 24000, "num_mels": 80, "fmin": 80, "fmax": 7600, "win_length": None,
             "window": "hann"}


def test_stage4_cli_without_a_vocoder_writes_griffin_lim_wavs(cuda, lib, tmp_path):
    from jatts_amd.bin import tts_decode
    from jatts_amd.models import FastSpeech2
    d = tmp_path
    _make_expdir(d)
    with open(d / "config.yml") as f:
        cfg = yaml.safe_load(f)
    del cfg["vocoder"]
    cfg.update(STFT_KEYS, griffin_lim_iters=4)
    with open(d / "config.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    np.savez(d / "stats.npz", mel_mean=np.full(80, -2.0, np.float32), mel_scale=np.full(80, 0.3, np.float32))
    args = ["--csv", str(d / "dev.csv"), "--stats", str(d / "stats.npz"), "--token-list", str(d / "tokens.txt"), "--token-column", "phonemes",
            "--checkpoint", str(d / "checkpoint-1steps.pkl"), "--outdir", str(d / "out"), "--verbose", "0", "--batch-size", "2"]
    tts_decode.main(args)
    model = FastSpeech2(**cfg["model_params"])
    model.load_state_dict(torch.load(d / "checkpoint-1steps.pkl", map_location="cpu")["model"])
    model = model.eval().to(cuda)
    items = tts_decode.read_items(str(d / "dev.csv"), "phonemes", tts_decode.TokenIDConverter(str(d / "tokens.txt")))
    olens = model.inference_batch([torch.from_numpy(it["token_indices"]).to(cuda) for it in items])["olens"]
    hop = STFT_KEYS["hop_size"]
    assert sorted(os.listdir(d / "out" / "wav")) == ["utt0.wav", "utt1.wav", "utt2.wav"]
    for i, n in enumerate(olens):
        with wave.open(str(d / "out" / "wav" / f"utt{i}.wav")) as w:
            assert (w.getframerate(), w.getsampwidth(), w.getnchannels()) == (24000, 2, 1) and w.getnframes() == int(n) * hop
            y = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        assert y[:-hop].any() and not y[-hop:].any()             # a waveform, then the 1-hop silent tail

    cfg.pop("fmax")                                              # a missing analysis key is named
    with open(d / "config.yml", "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(ValueError, match="'fmax'"):
        tts_decode.main(args)


def test_stage3_cli_without_a_vocoder_writes_intermediate_wavs(cuda, tmp_path):
    root = str(tmp_path)
    train, dev = corpora(root)
    conf = os.path.join(root, "fs2_gl.yaml")
    with open(conf, "w") as f:
        yaml.dump(fs2_config(train_max_steps=3, num_save_intermediate_results=1, griffin_lim_iters=2, **STFT_KEYS), f)
    outdir = os.path.join(root, "exp")
    r = cli(train, dev, conf, outdir)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    assert "No vocoder in the config: intermediate waveforms come from Griffin-Lim, 2 iterations." in log
    with wave.open(os.path.join(outdir, "predictions", "3steps", "wav", "0_gen.wav")) as w:
        assert w.getframerate() == 24000 and w.getsampwidth() == 2 and w.getnframes() % 256 == 0
