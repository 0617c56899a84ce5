"""GPU: stage 3 end to end on a toy corpus -- ``python -m jatts_amd.bin.tts_train`` (one run shared by the checks on its outputs, a resumed run,
a refused config), ``run_training`` in-process for the MAS models, and ``egs/jsut/tts1/run.sh --stage 2 --stop_stage 3``."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
from toy_corpus import TOKEN_LIST, write_corpus

pytestmark = pytest.mark.gpu

TRAIN_GEOM = [(3, 7), (2, 4), (5, 12), (4, 9), (2, 5), (6, 16), (3, 6)]
DEV_GEOM = [(4, 10), (2, 6), (3, 8), (5, 11)]
ENV = {**os.environ, "PYTHONPATH": ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")}


def fs2_config(**over):
    from jatts_amd.synthetic import FS2_SMALL
    cfg = {
        "feat_list": ["mel", "pitch", "energy"], "out_feat_type": "mel", "model_type": "FastSpeech2", "model_params": dict(FS2_SMALL),
        "trainer_type": "FastSpeech2Trainer", "collater_type": "FastSpeech2Collater",
        "criterions": {"MelLoss": {"_type": "L1Loss"}, "DurationPredictorLoss": {}, "PitchLoss": {}, "EnergyLoss": {}},
        "batch_size": 3, "pin_memory": True, "num_workers": 2, "allow_cache": True,
        "optimizer_type": "Adam", "optimizer_params": {"lr": 0.0008}, "grad_norm": 1.0, "scheduler": "warmuplr",
        "scheduler_params": {"warmup_steps": 4000},
        "train_max_steps": 6, "save_interval_steps": 3, "eval_interval_steps": 3, "log_interval_steps": 2, "num_save_intermediate_results": 2,
    }
    cfg.update(over)
    return cfg


def corpora(root, feat_list=("mel", "pitch", "energy"), durations=True):
    train = write_corpus(os.path.join(root, "train"), feat_list, durations, geom=TRAIN_GEOM, seed=1)
    dev = write_corpus(os.path.join(root, "dev"), feat_list, durations, geom=DEV_GEOM, seed=2, name="dev")
    return train, dev


def cli(train, dev, conf, outdir, *extra):
    cmd = [sys.executable, "-m", "jatts_amd.bin.tts_train", "--config", conf, "--train-csv", train["csv"], "--dev-csv", dev["csv"],
           "--stats", train["stats"], "--token-list", train["tokens"], "--token-column", "phonemes", "--outdir", outdir, "--seed", "3", *extra]
    return subprocess.run(cmd, env=ENV, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def trained(tmp_path_factory, cuda):
    root = str(tmp_path_factory.mktemp("stage3"))
    train, dev = corpora(root)
    conf = os.path.join(root, "fs2_small.yaml")
    with open(conf, "w") as f:
        yaml.dump(fs2_config(), f)
    outdir = os.path.join(root, "exp")
    r = cli(train, dev, conf, outdir)
    return {"root": root, "train": train, "dev": dev, "conf": conf, "outdir": outdir, "run": r}


def test_cli_trains_logs_evaluates_and_saves(trained, cuda):
    r, outdir = trained["run"], trained["outdir"]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    with open(os.path.join(outdir, "config.yml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    assert cfg["model_params"]["idim"] == len(TOKEN_LIST) and cfg["train_max_steps"] == 6
    from jatts_amd.models import FastSpeech2
    fresh = FastSpeech2(**cfg["model_params"])
    for steps in (3, 6):
        sd = torch.load(os.path.join(outdir, f"checkpoint-{steps}steps.pkl"), map_location="cpu")
        assert set(sd) == {"model", "optimizer", "scheduler", "steps", "epochs"} and sd["steps"] == steps
        assert list(sd["model"]) == list(fresh.state_dict())
    assert sd["epochs"] == 1                                  # 7 utterances, batches of 3: three steps an epoch (the short batch kept); as in the
                                                              # reference, the epoch in which the step limit is reached is not counted
    assert sorted(p for p in os.listdir(outdir) if p.endswith(".pkl")) == ["checkpoint-3steps.pkl", "checkpoint-6steps.pkl"]
    fresh.load_state_dict(sd["model"])
    fresh = fresh.to(cuda).eval()
    out = fresh.inference(torch.tensor([2, 3, 4, 5], device=cuda))
    assert out["feat_gen"].shape[1] == 80 and out["feat_gen"].shape[0] >= 1 and out["duration"].shape == (4,) and torch.isfinite(out["feat_gen"]).all()
    log = r.stdout + r.stderr
    for steps in (2, 4, 6):
        m = re.search(r"\(Steps: %d\) train/mel_loss = ([0-9.eE+-]+|nan|inf)\.\n" % steps, log)
        assert m and math.isfinite(float(m.group(1).rstrip("."))), steps
    ev = re.findall(r"\(Steps: (\d+)\) eval/(\w+) = ([0-9.eE+-]+|nan|inf)\.\n", log)
    assert {int(s) for s, _, _ in ev} == {3, 6} and {"mel_loss", "duration_loss", "pitch_loss", "energy_loss", "loss"} <= {k for _, k, _ in ev}
    assert all(math.isfinite(float(v.rstrip("."))) for _, _, v in ev)
    assert "pin_memory = True has no effect" in log and "No vocoder" in log
    rows = [json.loads(line) for line in open(os.path.join(outdir, "scalars.jsonl"))]
    assert {(x["steps"], x["tag"]) for x in rows} >= {(2, "train/loss"), (4, "train/loss"), (6, "train/loss"), (3, "eval/loss"), (6, "eval/loss")}
    lines = open(os.path.join(outdir, "predictions", "3steps", "durations", "0.txt")).read().split("\n")
    assert len(lines) == DEV_GEOM[0][0] + 1 and all(len(x.split(" ")) == 2 for x in lines[:-1])     # "<ground truth> <predicted>" per token
    assert os.path.exists(os.path.join(outdir, "predictions", "6steps", "durations", "1.txt"))
    assert not os.path.exists(os.path.join(outdir, "predictions", "3steps", "durations", "2.txt"))   # num_save_intermediate_results: 2


def test_resume_continues_to_the_step_limit(trained, tmp_path):
    assert trained["run"].returncode == 0
    out2 = str(tmp_path / "resumed")
    r = cli(trained["train"], trained["dev"], trained["conf"], out2, "--resume", os.path.join(trained["outdir"], "checkpoint-3steps.pkl"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(p for p in os.listdir(out2) if p.endswith(".pkl")) == ["checkpoint-6steps.pkl"]
    sd = torch.load(os.path.join(out2, "checkpoint-6steps.pkl"), map_location="cpu")
    assert sd["steps"] == 6 and float(sd["optimizer"]["state"][0]["step"]) == 6.0
    log = r.stdout + r.stderr
    assert "(Steps: 4) train/mel_loss" in log and "(Steps: 2) train/mel_loss" not in log and "Successfully resumed" in log


def test_unsupported_optimizer_is_refused_by_name(trained, tmp_path):
    conf = str(tmp_path / "sgd.yaml")
    with open(conf, "w") as f:
        yaml.dump(fs2_config(optimizer_type="SGD"), f)
    r = cli(trained["train"], trained["dev"], conf, str(tmp_path / "exp"))
    assert r.returncode != 0 and "optimizer_type" in r.stderr and "SGD" in r.stderr
    assert not os.path.exists(str(tmp_path / "exp" / "config.yml"))


@pytest.mark.parametrize("name,golden,feat_list,trainer", [("MatchaTTS_MAS", "matcha_mas_train_small.npz", ("mel",), "MatchaTTSTrainer"),
                                                           ("VITS", "vits_train_small.npz", ("mel", "spkemb"), "VITSTrainer")])
def test_run_training_in_process_for_the_mas_models(cuda, tmp_path, golden_dir, name, golden, feat_list, trainer):
    """Four loader-fed steps with a changing schedule (the forward-sum loss leaves after step 2, the duration loss joins at step 4) on the small
    configs of the training goldens: finite losses, logged from device scalars, a final checkpoint."""
    import logging
    import jatts_amd.models
    from jatts_amd import training
    from jatts_amd.data import BatchLoader, ResidentDataset
    train, dev = corpora(str(tmp_path), feat_list, durations=False)
    mk = lambda c: ResidentDataset(c["csv"], c["stats"], list(feat_list), c["tokens"], "phonemes", device=cuda)      # noqa: E731
    torch.manual_seed(0)
    model = getattr(jatts_amd.models, name)(idim=len(TOKEN_LIST), **json.loads(str(np.load(os.path.join(golden_dir, golden))["config"])))
    model = training.initialize_parameters(model).to(cuda)
    config = {"trainer_type": trainer, "model_type": name, "optimizer_params": {"lr": 1e-4}, "scheduler_type": "StepLR",
              "scheduler_params": {"step_size": 2, "gamma": 0.5}, "dp_train_start_steps": 2, "bin_loss_start_steps": 3, "lambda_align": 2.0,
              "train_max_steps": 4, "save_interval_steps": 100, "eval_interval_steps": 4, "log_interval_steps": 1, "num_save_intermediate_results": 1}
    cls, kw = training.trainer_kwargs(config)
    tr = cls(model, **kw)
    outdir = str(tmp_path / "exp")
    logging.getLogger().setLevel(logging.INFO)
    end = training.run_training(tr, BatchLoader(mk(train), 3, shuffle=True, seed=1), BatchLoader(mk(dev), 3, shuffle=False), config, outdir)
    assert end == {"steps": 4, "epochs": 1} and tr.steps == 4
    rows = [json.loads(line) for line in open(os.path.join(outdir, "scalars.jsonl"))]
    assert all(math.isfinite(x["value"]) for x in rows), [x for x in rows if not math.isfinite(x["value"])]
    tags = {(x["steps"], x["tag"]) for x in rows}
    assert {(s, "train/loss") for s in (1, 2, 3, 4)} <= tags and (4, "eval/loss") in tags
    assert (1, "train/forward_sum_loss") in tags and (4, "train/forward_sum_loss") not in tags
    assert (4, "train/duration_loss") in tags and (1, "train/duration_loss") not in tags
    sd = torch.load(os.path.join(outdir, "checkpoint-4steps.pkl"), map_location="cpu")
    assert sd["steps"] == 4 and list(sd["model"]) == list(model.state_dict())
    assert os.path.exists(os.path.join(outdir, "predictions", "4steps", "durations", "0.txt"))


def test_recipe_runs_stages_two_and_three(cuda, tmp_path):
    """egs/jsut/tts1/run.sh --stage 2 --stop_stage 3 on the toy layout: data/<set>.csv, data/<set>_raw_feat.csv, dump/train/stats.npz ->
    dump/token_list/train_phn_julius/tokens.txt, exp/<expname>/{config.yml,stats.npz,tokens.txt,checkpoint-2steps.pkl,train.log}."""
    import shutil
    root = str(tmp_path)
    train, dev = corpora(os.path.join(root, "src"))
    os.makedirs(os.path.join(root, "data"))
    os.makedirs(os.path.join(root, "dump", "train"))
    os.makedirs(os.path.join(root, "conf"))
    shutil.copy(train["csv"], os.path.join(root, "data", "train.csv"))
    shutil.copy(train["csv"], os.path.join(root, "data", "train_raw_feat.csv"))
    shutil.copy(dev["csv"], os.path.join(root, "data", "dev_raw_feat.csv"))
    shutil.copy(train["stats"], os.path.join(root, "dump", "train", "stats.npz"))
    with open(os.path.join(root, "conf", "toy.yaml"), "w") as f:
        yaml.dump(fs2_config(train_max_steps=2, save_interval_steps=100, eval_interval_steps=100, log_interval_steps=1), f)
    r = subprocess.run(["bash", os.path.join(ROOT, "egs", "jsut", "tts1", "run.sh"), "--stage", "2", "--stop_stage", "3", "--conf", "conf/toy.yaml"],
                       cwd=root, env={**ENV, "PYTHON": sys.executable}, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    toks = open(os.path.join(root, "dump", "token_list", "train_phn_julius", "tokens.txt"), encoding="utf-8").read().split("\n")[:-1]
    assert toks[:2] == ["<blank>", "<unk>"] and toks[-1] == "<sos/eos>" and set(toks[2:-1]) == {p for row in train["rows"] for p in row["phonemes"].split(" ")}
    exp = os.path.join(root, "exp", "train_phn_none_toy")
    for name in ("config.yml", "stats.npz", "tokens.txt", "checkpoint-2steps.pkl", "train.log"):
        assert os.path.exists(os.path.join(exp, name)), (name, os.listdir(exp))
    assert "(Steps: 2) train/loss" in open(os.path.join(exp, "train.log")).read()
    assert "run them there" not in r.stdout.split("Stage 2")[1]


def test_recipe_runs_stages_one_to_four_in_one_call(cuda, tmp_path, golden_dir):
    """egs/jsut/tts2/run.sh --stage 1 --stop_stage 4 on this package alone, given stage 0's csv files: wav files -> dumps and statistics ->
    token list -> a trained MatchaTTS_MAS checkpoint (with a vocoder in the config: the intermediate waveform is written too) -> decoded wav."""
    import wave
    from jatts_amd.synthetic import HIFIGAN_V1_24K, synth_hifigan_state
    from test_preprocess_cli_gpu import CONF, _write_csv, _write_toy_data
    work = tmp_path / "recipe"
    for sub in ("data", "conf", "wav", "downloads/hfg"):
        os.makedirs(work / sub)
    rows = _write_toy_data(work / "wav")                         # utt0, utt1, utt2 and one that clips (stage 1 drops it)
    for name, rs in {"train": rows, "dev": rows[:2], "test": rows[2:3]}.items():
        _write_csv(work / "data" / f"{name}.csv", rs)
    vparams = dict(HIFIGAN_V1_24K, channels=512)
    v = work / "downloads" / "hfg"
    torch.save({"model": {"generator": synth_hifigan_state(vparams, 0)}}, v / "voc.pkl")
    with open(v / "voc.yml", "w") as f:
        yaml.safe_dump({"sampling_rate": 24000, "generator_type": "HiFiGANGenerator",
                        "generator_params": {k: (list(x) if isinstance(x, tuple) else x) for k, x in vparams.items()}}, f)
    np.savez(v / "vstats.npz", mean=np.zeros(80, np.float32), scale=np.ones(80, np.float32))
    conf = dict(CONF, hop_size=300, out_feat_type="mel", model_type="MatchaTTS_MAS", trainer_type="MatchaTTSTrainer",
                model_params=json.loads(str(np.load(os.path.join(golden_dir, "matcha_mas_train_small.npz"))["config"])),
                collater_type="FastSpeech2Collater", criterions={"CFMLoss": {}, "EncoderPriorLoss": {}, "ForwardSumLoss": {}, "DurationPredictorLoss": {}},
                lambda_align=2.0, temperature=0.667, ode_steps=2, batch_size=2, optimizer_type="Adam", optimizer_params={"lr": 1e-4},
                grad_norm=1.0, scheduler_type="StepLR", scheduler_params={"step_size": 10, "gamma": 0.5}, dp_train_start_steps=1,
                bin_loss_start_steps=1, train_max_steps=2, save_interval_steps=100, eval_interval_steps=2, log_interval_steps=1,
                num_save_intermediate_results=1,
                vocoder={"checkpoint": "downloads/hfg/voc.pkl", "config": "downloads/hfg/voc.yml", "stats": "downloads/hfg/vstats.npz"})
    (work / "conf" / "toy.yaml").write_text(yaml.safe_dump(conf))
    r = subprocess.run(["bash", os.path.join(ROOT, "egs", "jsut", "tts2", "run.sh"), "--stage", "1", "--stop_stage", "4", "--conf", "conf/toy.yaml",
                        "--preprocess_batch_size", "4", "--decode_batch_size", "2", "--train_seed", "0"], cwd=work,
                       env={**ENV, "PYTHON": sys.executable}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for stage in ("Stage 1: Feature extraction", "Stage 2: Token list generation", "Stage 3: Network training", "Stage 4: Network decoding"):
        assert stage in r.stdout, stage
    exp = work / "exp" / "train_phn_none_toy"
    assert (work / "dump" / "train" / "stats.npz").exists() and (work / "dump" / "token_list" / "train_phn_pyopenjtalk" / "tokens.txt").exists()
    assert (exp / "tokens.txt").read_text().split("\n") == ["<blank>", "<unk>", "a", "b", "<sos/eos>", ""]
    sd = torch.load(exp / "checkpoint-2steps.pkl", map_location="cpu")
    assert sd["steps"] == 2
    log = (exp / "train.log").read_text()
    assert "(Steps: 2) train/loss" in log and "(Steps: 2) eval/loss" in log and "The number of training files = 3." in log
    with wave.open(str(exp / "predictions" / "2steps" / "wav" / "0_gen.wav")) as w:          # the vocoder branch of the intermediate results
        assert w.getframerate() == 24000 and w.getnframes() % 300 == 0 and w.getnframes() > 0
    with wave.open(str(exp / "results" / "checkpoint-2steps" / "test" / "wav" / "utt2.wav")) as w:
        assert w.getframerate() == 24000 and w.getnframes() % 300 == 0 and w.getnframes() > 0


def test_world_size_two_trains_one_model(trained, tmp_path):
    """``tts_train`` as two data-parallel ranks (child processes sharing this box's GPU, exchange over gloo), UNSEEDED: every rank draws its own
    initial parameters, the broadcast from rank 0 makes them one model, DistributedSampler deals the utterances, the averaged gradients keep
    the replicas identical to the last step (spread 0), rank 0 writes the checkpoints."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    train, dev, out = trained["train"], trained["dev"], str(tmp_path / "exp")
    conf = str(tmp_path / "w2.yaml")
    with open(conf, "w") as f:
        yaml.dump(fs2_config(train_max_steps=3, save_interval_steps=100, eval_interval_steps=2, log_interval_steps=1), f)
    cmd = [sys.executable, "-m", "jatts_amd.bin.tts_train", "--config", conf, "--train-csv", train["csv"], "--dev-csv", dev["csv"], "--stats",
           train["stats"], "--token-list", train["tokens"], "--token-column", "phonemes", "--outdir", out]
    procs = [subprocess.Popen(cmd, env={**ENV, "RANK": str(r), "LOCAL_RANK": "0", "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
                                        "JATTS_SHARED_GPU": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"},
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=240)
            assert p.returncode == 0, o[-2000:] + e[-3000:]
            logs.append(o + e)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert "World size: 2" in logs[0] and "Replica spread of the parameter sum over 2 ranks at exit: 0.000e+00." in logs[0]
    assert "(Steps: 3) train/loss" in logs[0] and "(Steps: 2) eval/loss" in logs[0] and "train/loss" not in logs[1]       # rank 0 logs
    assert sorted(p for p in os.listdir(out) if p.endswith(".pkl")) == ["checkpoint-3steps.pkl"]
    sd = torch.load(os.path.join(out, "checkpoint-3steps.pkl"), map_location="cpu")
    assert sd["steps"] == 3 and sd["epochs"] == 1          # 7 utterances over 2 ranks: 4 each, two batches of up to 3 an epoch
