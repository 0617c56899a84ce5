"""CPU: the host side of stages 2 and 3 -- the token-list order rule, the config -> trainer mapping and its refusals, the loader's batch
geometry from a host index, and the jatts_collate entry of the C ABI (exported, prototyped, mirrored; its argument checks run before any
HIP call, so they answer without a GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_token_list_order_and_add_symbol_placement(tmp_path):
    from jatts_amd.bin import generate_token_list as g
    rows = ["b a c a", "c b a  d", "e"]              # a: 3, b: 2, c: 2, d: 1, e: 1; ties in first-appearance order; the double space is no token
    assert g.build_token_list(rows) == ["a", "b", "c", "d", "e"]
    assert g.build_token_list(rows, ["<blank>:0", "<unk>:1", "<sos/eos>:-1"]) == ["<blank>", "<unk>", "a", "b", "c", "d", "e", "<sos/eos>"]
    assert g.build_token_list(rows, ["<x>:2"]) == ["a", "b", "<x>", "c", "d", "e"]
    assert g.build_token_list(rows, ["<x>:-2"]) == ["a", "b", "c", "d", "<x>", "e"]
    with pytest.raises(RuntimeError, match="Format error"):
        g.build_token_list(rows, ["<blank>"])
    csv_path, out = tmp_path / "t.csv", tmp_path / "sub" / "tokens.txt"
    csv_path.write_text("sample_id,phonemes\nu0,b a c a\nu1,c b a  d\nu2,e\n", encoding="utf-8")
    base = ["--csv", str(csv_path), "--out", str(out), "--column", "phonemes", "--non_linguistic_symbols", "none"]
    g.main(base + ["--cleaner", "none", "--add_symbol", "<blank>:0", "--add_symbol", "<unk>:1", "--add_symbol", "<sos/eos>:-1"])
    assert out.read_text(encoding="utf-8").split("\n") == ["<blank>", "<unk>", "a", "b", "c", "d", "e", "<sos/eos>", ""]
    for flags, word in ((["--cleaner", "jaconv"], "cleaner"), (["--g2p", "pyopenjtalk"], "g2p"), (["--token_type", "char"], "token_type"),
                        (["--token_type", "word"], "token_type")):
        with pytest.raises(ValueError, match=word):
            g.main(base + flags)


FS2_CONFIG = {
    "trainer_type": "FastSpeech2Trainer", "optimizer_type": "Adam", "optimizer_params": {"lr": 0.0008}, "grad_norm": 1.0,
    "scheduler_params": {"warmup_steps": 4000},
    "criterions": {"MelLoss": {"_type": "L1Loss"}, "DurationPredictorLoss": {}, "PitchLoss": {}, "EnergyLoss": {}},
    "pin_memory": True, "num_workers": 2, "allow_cache": True,
}


def test_config_maps_onto_the_trainers_keyword_arguments():
    from jatts_amd import training as t
    cls, kw = t.trainer_kwargs(FS2_CONFIG)
    assert cls is t.FastSpeech2Trainer
    assert kw == {"lr": 0.0008, "grad_norm": 1.0, "scheduler": "warmuplr", "warmup_steps": 4000, "gradient_accumulate_steps": 1}
    matcha = {"trainer_type": "MatchaTTSTrainer", "optimizer_params": {"lr": 1e-4, "betas": [0.8, 0.99], "eps": 1e-9, "weight_decay": 0.01},
              "grad_norm": 0.5, "scheduler_type": "StepLR", "scheduler_params": {"step_size": 10000, "gamma": 0.5}, "lambda_align": 2.0,
              "dp_train_start_steps": 10000, "bin_loss_start_steps": 15000,
              "criterions": {"CFMLoss": {}, "EncoderPriorLoss": {}, "ForwardSumLoss": {}, "DurationPredictorLoss": {}}}
    cls, kw = t.trainer_kwargs(matcha)
    assert cls is t.MatchaTTSTrainer
    assert kw == {"lr": 1e-4, "betas": (0.8, 0.99), "eps": 1e-9, "weight_decay": 0.01, "grad_norm": 0.5, "scheduler": "steplr",
                  "scheduler_params": {"step_size": 10000, "gamma": 0.5}, "gradient_accumulate_steps": 1, "lambda_align": 2.0,
                  "dp_train_start_steps": 10000, "bin_loss_start_steps": 15000}
    vits = {"trainer_type": "VITSTrainer", "optimizer_params": {"lr": 0.0008}, "scheduler_params": {"warmup_steps": 4000},
            "gradient_accumulate_steps": 4, "lambda_align": 2.0, "lambda_mel": 10.0, "dp_train_start_steps": 1, "bin_loss_start_steps": 2,
            "criterions": {"MelLoss": {"_type": "L1Loss"}, "KLDivergenceLoss": {}, "ForwardSumLoss": {}, "DurationPredictorLoss": {}}}
    cls, kw = t.trainer_kwargs(vits)
    assert cls is t.VITSTrainer and kw["gradient_accumulate_steps"] == 4 and kw["lambda_mel"] == 10.0 and kw["lambda_align"] == 2.0
    assert set(t.NO_EFFECT_KEYS) == {"pin_memory", "num_workers", "allow_cache"}
    # the schedules the mapping selects are the trainers' own
    assert t.scheduled_lr("steplr", 1e-4, 10001, step_size=10000, gamma=0.5) == 5e-5


@pytest.mark.parametrize("change,word", [
    ({"optimizer_type": "SGD"}, "optimizer_type"),
    ({"optimizer_params": {"lr": 1e-3, "amsgrad": True}}, "amsgrad"),
    ({"scheduler_type": "exponentiallr"}, "scheduler_type"),
    ({"scheduler_params": {"warmup_steps": 10, "gamma": 0.1}}, "gamma"),
    ({"scheduler_type": "StepLR", "scheduler_params": {"gamma": 0.5}}, "step_size"),
    ({"trainer_type": "VALLETrainer"}, "trainer_type"),
    ({"freeze_modules": ["encoder"]}, "freeze_modules"),
    ({"criterions": {"MelLoss": {"_type": "L2Loss"}}}, "MelLoss._type"),
    ({"criterions": {"PitchLoss": {"use_masking": False}}}, "PitchLoss.use_masking"),
    ({"criterions": {"DurationPredictorLoss": {"offset": 0.5}}}, "DurationPredictorLoss.offset"),
    ({"criterions": {"EnergyLoss": {"reduction": "sum"}}}, "EnergyLoss.reduction"),
    ({"criterions": {"KLDivergenceLoss": {}}}, "KLDivergenceLoss"),
    ({"criterions": {"GuidedAttentionLoss": {}}}, "GuidedAttentionLoss"),
    ({"lambda_mel": 10.0}, "lambda_mel"),
    ({"feat_list": ["mel", "energy"]}, "'pitch'"),
    ({"feat_list": ["mel", "pitch"]}, "'energy'"),
    ({"trainer_type": "VITSTrainer", "criterions": {}, "feat_list": ["mel"]}, "'spkemb'"),
    ({"dp_train_start_steps": 100}, "dp_train_start_steps"),
])
def test_what_the_trainers_cannot_do_is_refused_by_name(change, word):
    from jatts_amd import training as t
    with pytest.raises(ValueError, match=re.escape(word)):
        t.trainer_kwargs({**FS2_CONFIG, **change})


def test_batch_geometry_from_a_host_index():
    from jatts_amd.data import batch_geometry
    index = {"tokens": np.array([3, 1, 5, 4], dtype=np.int32), "mel": np.array([7, 1, 12, 9], dtype=np.int32),
             "spkemb": np.array([1, 1, 1, 1], dtype=np.int32)}
    lens, t_max = batch_geometry(index, [2, 0])
    assert lens["tokens"].tolist() == [5, 3] and lens["mel"].tolist() == [12, 7] and lens["tokens"].dtype == np.int64
    assert t_max == {"tokens": 5, "mel": 12, "spkemb": 1}
    lens, t_max = batch_geometry(index, [1])
    assert t_max == {"tokens": 1, "mel": 1, "spkemb": 1} and lens["mel"].tolist() == [1]
    lens, t_max = batch_geometry(index, [3, 3, 0])
    assert lens["mel"].tolist() == [9, 9, 7] and t_max["tokens"] == 4


def test_collate_entry_is_exported_prototyped_and_mirrored(lib):
    import ctypes as C
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    assert hasattr(lib, "jatts_collate") and "jatts_collate" in _abi.PROTOTYPES
    assert _abi.PROTOTYPES["jatts_collate"] == (C.c_int, [C.POINTER(_abi.CollateField), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p])
    body = re.search(r"typedef struct jatts_collate_field \{(.*?)\} jatts_collate_field;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"([a-z_0-9]+)(?:\[\d+\])?\s*;", body) == [f[0] for f in _abi.CollateField._fields_]
    assert C.sizeof(_abi.CollateField) == 48          # four pointers, three int32, padded to 8
    assert int(re.search(r"#define JATTS_COLLATE_MAX_FIELDS (\d+)", hdr).group(1)) == _abi.COLLATE_MAX_FIELDS == 8
    for cite in ("jatts/datasets/tts_dataset.py:69-145", "jatts/collaters/fastspeech2.py:17-107"):
        assert cite in hdr, cite
    assert int(re.search(r"#define JATTS_ABI_VERSION (\d+)", hdr).group(1)) == _abi.ABI_VERSION == lib.jatts_abi_version()
    mk = open(os.path.join(ROOT, "jatts_amd", "csrc", "Makefile")).read()
    assert "collate.hip" in mk


def test_collate_argument_checks_answer_before_any_launch(lib):
    """JATTS_ERR_ARG (-1) for every malformed call; the pointers are never dereferenced on these paths (there is no device here)."""
    from jatts_amd import _abi
    good = (64, 64, 64, 64, 4, 5, 7)

    def call(field=good, n_fields=1, utt=64, n_batch=1, count=1):
        tab = (_abi.CollateField * count)(*[_abi.CollateField(*field)] * count)
        return lib.jatts_collate(tab, n_fields, utt, n_batch, None)

    assert call(n_fields=0) == -1 and call(n_fields=9, count=9) == -1 and b"n_fields" in lib.jatts_last_error()
    assert call(n_batch=0) == -1 and call(utt=None) == -1
    for pos, v in ((4, 2), (4, 16), (5, 0), (6, 0), (0, None), (1, None), (2, None), (3, None)):
        f = list(good)
        f[pos] = v
        assert call(tuple(f)) == -1, (pos, v)
    assert call((64, 64, 64, 64, 2, 5, 7)) == -1 and b"elem_bytes" in lib.jatts_last_error()


def test_recipes_run_stages_two_and_three_here():
    import glob
    scripts = sorted(glob.glob(os.path.join(ROOT, "egs", "*", "tts*", "run.sh")))
    assert len(scripts) == 6
    for s in scripts:
        t = open(s).read()
        assert "egs/common/stage3.sh" in t and "stage2_tokens" in t and "stage3_train" in t and "run them there\"" not in t.split("Stage 1")[1].split("Stage 4")[0], s
        assert "\nstage=4 " in t and "\nstop_stage=4 " in t, s
    sh = open(os.path.join(ROOT, "egs", "common", "stage3.sh")).read()
    for word in ("jatts_amd.bin.generate_token_list", "jatts_amd.bin.tts_train", "torch.distributed.run", "--add_symbol", "train.log", "tokens.txt"):
        assert word in sh, word


def test_initialize_parameters_leaves_what_the_reference_constructors_leave():
    """The model classes are built all-zero; a from-scratch run starts from the reference's distributions (modules/initialize.py:70-95)."""
    import json
    import torch
    import jatts_amd.models as M
    from jatts_amd import training as t
    from jatts_amd.synthetic import FS2_SMALL
    golden = os.path.join(ROOT, "tests", "golden")
    cfgs = {"FastSpeech2": dict(FS2_SMALL, spk_embed_dim=16),
            "MatchaTTS_MAS": json.loads(str(np.load(os.path.join(golden, "matcha_mas_train_small.npz"))["config"])),
            "VITS": json.loads(str(np.load(os.path.join(golden, "vits_train_small.npz"))["config"]))}
    for name, cfg in cfgs.items():
        m = getattr(M, name)(idim=200, **cfg)
        assert all(float(p.abs().sum()) == 0.0 for p in m.parameters()), name
        torch.manual_seed(0)
        t.initialize_parameters(m, "xavier_uniform")
        for k, p in m.named_parameters():
            if p.dim() > 1:
                assert float(p.abs().sum()) > 0.0 and torch.isfinite(p).all(), k
                if k not in t._EMBEDDING_TABLES:
                    fan_in, fan_out = torch.nn.init._calculate_fan_in_and_fan_out(p)
                    assert float(p.abs().max()) <= (6.0 / (fan_in + fan_out)) ** 0.5 + 1e-7, k
            elif k.endswith(".bias") or k.endswith((".alpha", ".beta")):
                assert float(p.abs().sum()) == 0.0, k
            else:
                assert k.endswith(".weight") and bool((p == 1).all()), k
        emb = dict(m.named_parameters())["text_encoder.emb.weight" if name == "VITS" else "encoder.embed.0.weight"]
        assert 0.9 < float(emb[1:].std()) < 1.1 and (name == "VITS" or float(emb[0].abs().sum()) == 0.0)
        for k, b in m.named_buffers():
            if k.endswith("running_var"):
                assert bool((b == 1).all()), k
    with pytest.raises(ValueError, match="init_type"):
        t.initialize_parameters(m, "pytorch")


def test_start_up_checks_on_the_data_and_on_keys_nobody_reads():
    from jatts_amd import training as t
    assert t.trainer_kwargs({**FS2_CONFIG, "feat_list": ["mel", "pitch", "energy"]})[0] is t.FastSpeech2Trainer
    for ttype, mtype, has, ok in (("FastSpeech2Trainer", "FastSpeech2", False, False), ("FastSpeech2Trainer", "FastSpeech2", True, True),
                                  ("MatchaTTSTrainer", "MatchaTTS", False, False), ("MatchaTTSTrainer", "MatchaTTS_MAS", False, True),
                                  ("VITSTrainer", "VITS", False, True)):
        cfg = {"trainer_type": ttype, "model_type": mtype}
        if ok:
            t.check_durations(cfg, has)
        else:
            with pytest.raises(ValueError, match="durations"):
                t.check_durations(cfg, has)
    cfg = {**FS2_CONFIG, "scheduler": "warmuplr", "sampling_rate": 24000, "hop_size": 300, "train_max_steps": 10, "outdir": "x", "typo_interval_steps": 5}
    assert t.unread_keys(cfg, cli_keys=["outdir"]) == ["scheduler", "typo_interval_steps"]


def test_initialiser_name_rules_match_the_models_schemas():
    """Which tensors ``initialize_parameters`` treats as embedding tables and which as norm scales, spelled out against the three schemas: a
    new parameter that a suffix rule would catch by accident fails here."""
    import json
    import jatts_amd.models as M
    from jatts_amd import training as t
    from jatts_amd.synthetic import FS2_SMALL
    golden = os.path.join(ROOT, "tests", "golden")
    cfgs = {"FastSpeech2": (dict(FS2_SMALL, spk_embed_dim=16), {"encoder.embed.0.weight"}),
            "MatchaTTS_MAS": (json.loads(str(np.load(os.path.join(golden, "matcha_mas_train_small.npz"))["config"])), {"encoder.embed.0.weight"}),
            "MatchaTTS": (json.loads(str(np.load(os.path.join(golden, "matcha_tts1_train_small.npz"))["config"])), {"encoder.embed.0.weight"}),
            "VITS": (json.loads(str(np.load(os.path.join(golden, "vits_train_small.npz"))["config"])), {"text_encoder.emb.weight"})}
    norm = re.compile(r"(^|\.)(norm\w*|after_norm|layer_norm|ln\w*|\d+)\.weight$")
    for name, (cfg, tables) in cfgs.items():
        m = getattr(M, name)(idim=37, **cfg)
        P = dict(m.named_parameters())
        assert {k for k, p in P.items() if p.dim() == 2 and k in t._EMBEDDING_TABLES} == tables, name
        assert not any("emb" in k and p.dim() == 2 and p.shape[0] == 37 for k, p in P.items() if k not in tables), name     # no table is missed
        assert all(P[k].shape[0] == 37 and P[k].dim() == 2 for k in tables), name
        scales = [k for k, p in P.items() if p.dim() == 1 and k.endswith(".weight")]
        assert scales and all(norm.search(k) for k in scales), [k for k in scales if not norm.search(k)]
        assert all(P[k[:-len("weight")] + "bias"].shape == P[k].shape for k in scales), name       # a scale comes with a shift of its size
