"""CPU: the ABI of training on the fp32_bf16x3 arithmetic (round 7) -- the two new entry points are declared, bound and exported -- and the
trainers' accepted precisions -- and the trainers' arithmetic: the precision.TrainArithmetic table, the autograd.arithmetic context, the conv code helper
(pure Python: no GPU, no library)."""
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


def test_train_arithmetic_table():
    """precision.train_arithmetic: every pair of accepted names -> its record; a record passes through; anything else raises, naming every accepted value."""
    from jatts_amd import _abi, precision
    from jatts_amd.precision import TrainArithmetic, train_arithmetic
    operand = {"fp32": _abi.F32, "fp32_split": _abi.F32S, "fp32_bf16x3": _abi.F32E}
    attention = {None: _abi.F32, "fp32": _abi.F32, "fp32_bf16x3": _abi.F32E}
    assert set(precision.TRAIN_PRECISIONS) == set(operand) and set(precision.TRAIN_ATTENTIONS) == set(attention) - {None}
    for p, op in operand.items():
        for a, at in attention.items():
            assert train_arithmetic(p, a) == TrainArithmetic(op, at), (p, a)
    assert train_arithmetic() == TrainArithmetic(_abi.F32, _abi.F32)
    rec = TrainArithmetic(_abi.F32S, _abi.F32E)
    assert train_arithmetic(rec) is rec
    for bad in ("fp16", "fp32_bf16x3_6p"):
        with pytest.raises(ValueError) as e:
            train_arithmetic(bad)
        assert all(repr(p) in str(e.value) and d in str(e.value) for p, d in precision.TRAIN_PRECISIONS.items()), str(e.value)
    with pytest.raises(ValueError) as e:
        train_arithmetic("fp32", "bf16")
    assert "None" in str(e.value) and all(repr(a) in str(e.value) and d in str(e.value) for a, d in precision.TRAIN_ATTENTIONS.items()), str(e.value)


def test_arithmetic_context_sets_nests_and_restores():
    from jatts_amd import _abi
    from jatts_amd.autograd import arithmetic, current_arithmetic
    from jatts_amd.precision import TrainArithmetic
    exact = TrainArithmetic(_abi.F32, _abi.F32)
    assert current_arithmetic() == exact
    with arithmetic("fp32_bf16x3", attention="fp32_bf16x3"):
        assert current_arithmetic() == TrainArithmetic(_abi.F32E, _abi.F32E)
        with arithmetic("fp32_split"):          # the inner record replaces the outer whole: the attention is exact again
            assert current_arithmetic() == TrainArithmetic(_abi.F32S, _abi.F32)
        assert current_arithmetic() == TrainArithmetic(_abi.F32E, _abi.F32E)
        with arithmetic(TrainArithmetic(_abi.F32, _abi.F32E)):
            assert current_arithmetic() == TrainArithmetic(_abi.F32, _abi.F32E)
    assert current_arithmetic() == exact
    with pytest.raises(RuntimeError, match="inside"):
        with arithmetic("fp32_split"):
            assert current_arithmetic().operand == _abi.F32S
            raise RuntimeError("inside")
    assert current_arithmetic() == exact
    with pytest.raises(ValueError):             # a bad name never enters
        with arithmetic("fp16"):
            pass
    assert current_arithmetic() == exact


ANY_SHAPES = [(1, 512, 2048, 4096), (3, 384, 384, 300), (5, 64, 72, 7)]          # (k, c_in, n_out, rows)


def test_conv_codes_table(monkeypatch):
    """autograd.conv_codes(operand, k, dil, c_in, n_out, rows) -> (conv code, weight-gradient code): the one place that combines hip.conv_halo_fits
    and emul_wgrad_wins."""
    from jatts_amd import _abi, autograd
    F32, F32S, F32E = _abi.F32, _abi.F32S, _abi.F32E
    for k, c_in, n_out, rows in ANY_SHAPES:
        for dil in (1, 16, 17, 40):
            assert autograd.conv_codes(F32, k, dil, c_in, n_out, rows) == (F32, F32)
    for c_in, n_out, rows in [s[1:] for s in ANY_SHAPES]:
        assert autograd.conv_codes(F32S, 3, 16, c_in, n_out, rows) == (F32S, F32)       # halo 32
        assert autograd.conv_codes(F32S, 3, 17, c_in, n_out, rows) == (F32, F32)        # halo 34
        assert autograd.conv_codes(F32E, 3, 17, c_in, n_out, rows) == (F32, F32)
        assert autograd.conv_codes(F32E, 5, 9, c_in, n_out, rows) == (F32, F32)         # halo 36
    assert autograd.emul_wgrad_wins(512, 2048, 1, 4096) and not autograd.emul_wgrad_wins(384, 384, 3, 4096)
    assert autograd.conv_codes(F32E, 1, 1, 512, 2048, 4096) == (F32E, F32E)
    assert autograd.conv_codes(F32E, 3, 1, 384, 384, 4096) == (F32E, F32)
    assert autograd.conv_codes(F32E, 3, 16, 384, 384, 4096) == (F32E, F32)
    # the rule is looked up at call time, and a halo that does not fit never reaches it
    monkeypatch.setattr(autograd, "emul_wgrad_wins", lambda c_in, n_out, k, rows: True)
    assert autograd.conv_codes(F32E, 3, 16, 384, 384, 4096) == (F32E, F32E)
    assert autograd.conv_codes(F32E, 3, 17, 384, 384, 4096) == (F32, F32)
    assert autograd.conv_codes(F32S, 3, 16, 384, 384, 4096) == (F32S, F32)


def test_autograd_does_not_import_training():
    """A fresh interpreter that imports jatts_amd.autograd has not imported jatts_amd.training (no cycle: training imports autograd, never the reverse)."""
    import subprocess
    import sys
    code = "import sys, jatts_amd.autograd; print('jatts_amd.training' in sys.modules, 'jatts_amd.autograd' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["False", "True"], out.stdout + out.stderr
