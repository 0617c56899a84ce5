"""CPU: the ABI of training on the fp32_bf16x3 arithmetic (round 7) -- the two new entry points are declared, bound and exported -- and the
trainers' accepted precisions."""
import os
import re

import pytest

from conftest import ROOT


def test_emulated_training_entry_points_are_declared_bound_and_exported(lib):
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    for name in ("jatts_pack_conv_weight_bf16x3", "jatts_conv1d_wgrad_emul"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    # same argument list as the exact-f32 weight gradient plus the dtype code
    assert len(_abi.PROTOTYPES["jatts_conv1d_wgrad_emul"][1]) == len(_abi.PROTOTYPES["jatts_conv1d_wgrad"][1]) + 1


def test_trainer_precisions():
    """FastSpeech2Trainer.__init__ (and with it the Matcha / VITS trainers, which pass **kw up) checks the precision before it touches the model: the three
    accepted names, and a message that lists them for anything else."""
    from jatts_amd import training
    assert tuple(training.TRAIN_PRECISIONS) == ("fp32", "fp32_split", "fp32_bf16x3")
    for cls in (training.FastSpeech2Trainer, training.MatchaTTSTrainer, training.VITSTrainer):
        for bad in ("fp32_bf16x3_6p", "fp16"):
            with pytest.raises(ValueError) as e:
                cls(None, precision=bad)
            assert all(repr(p) in str(e.value) for p in ("fp32", "fp32_split", "fp32_bf16x3")), str(e.value)


def test_conv_mode_switches_are_independent():
    from jatts_amd import training
    assert training.SPLIT_CONVS[0] is False and training.EMUL_CONVS[0] is False
    with training.emul_convs():
        assert training.EMUL_CONVS[0] and not training.SPLIT_CONVS[0]
        with training.split_convs(True):
            assert training.EMUL_CONVS[0] and training.SPLIT_CONVS[0]
    with training.precision_convs("fp32_split"):
        assert training.SPLIT_CONVS[0] and not training.EMUL_CONVS[0]
    with training.precision_convs("fp32_bf16x3"):
        assert training.EMUL_CONVS[0] and not training.SPLIT_CONVS[0]
    assert training.SPLIT_CONVS[0] is False and training.EMUL_CONVS[0] is False
