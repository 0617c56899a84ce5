"""CPU: the self-attention arithmetic as a switch of its own -- set_precision(precision, attention=None) on the four model classes (which pairs
are accepted, what the default leaves alone, what re-keys the prepared state), the routing rule's signature, the decode CLI's flag, and the ABI
version the JATTS_F32E attention arrived with.  No GPU is touched: the models are only constructed."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT

F32_PRECISIONS = ["fp32", "fp32_bf16x3", "fp32_bf16x3_6p", "fp32_split"]


def _models(golden_dir):
    from jatts_amd.models import VITS, FastSpeech2, MatchaTTS, MatchaTTS_MAS
    from jatts_amd.synthetic import FS2_SMALL
    small = lambda name: json.loads(str(np.load(os.path.join(golden_dir, name))["config"]))  # noqa: E731
    mcfg = small("matcha_small.npz")
    out = [FastSpeech2(idim=20, **FS2_SMALL), MatchaTTS_MAS(idim=20, **mcfg), VITS(idim=20, **small("vits_small.npz"))]
    try:
        out.append(MatchaTTS(idim=20, **mcfg))
    except TypeError:      # (the duration-supervised class takes a subset of the MAS config)
        sig = inspect.signature(MatchaTTS.__init__).parameters
        out.append(MatchaTTS(idim=20, **{k: v for k, v in mcfg.items() if k in sig}))
    return out


def test_set_precision_accepts_and_rejects_attention_choices(golden_dir):
    for m in _models(golden_dir):
        name = type(m).__name__
        assert m.precision == "fp32" and m.attention is None, name
        for prec in F32_PRECISIONS:
            for att in (None, "fp32", "fp32_bf16x3"):
                assert m.set_precision(prec, attention=att) is m, (name, prec, att)
                assert m.precision == prec and m.attention == att, (name, prec, att)
        m.set_precision("fp16")
        assert m.precision == "fp16" and m.attention is None
        for att in ("fp32", "fp32_bf16x3"):
            with pytest.raises(ValueError):
                m.set_precision("fp16", attention=att)
        for att in ("fp16", "fp32_split", "fp32_bf16x3_6p", "bf16x3", "", 3):
            with pytest.raises(ValueError):
                m.set_precision("fp32_bf16x3", attention=att)
        with pytest.raises(ValueError):
            m.set_precision("nope", attention="fp32")
        assert m.precision == "fp16" and m.attention is None, f"{name}: a refused call must leave the model as it was"


def test_default_leaves_precision_and_attention_as_today(golden_dir):
    for m in _models(golden_dir):
        m.set_precision("fp32_bf16x3")
        assert (m.precision, m.attention) == ("fp32_bf16x3", None)
        m._prep = {"key": "sentinel"}
        m.set_precision("fp32_bf16x3")                       # nothing changed: the prepared state stays
        m.set_precision("fp32_bf16x3", attention=None)
        assert m._prep == {"key": "sentinel"}
        m.set_precision("fp32_bf16x3", attention="fp32_bf16x3")      # the attention choice alone re-keys it
        assert m._prep is None and m.attention == "fp32_bf16x3"
        m._prep = {"key": "sentinel"}
        m.set_precision("fp32_bf16x3")                       # ... and the plain call goes back to the default
        assert m._prep is None and m.attention is None


def test_attention_dtype_routing_is_a_function_of_head_geometry_only():
    from jatts_amd import hip
    assert list(inspect.signature(hip.emul_attention_wins).parameters) == ["n_heads", "d_k", "rel_mode"]
    for H, dk, rel in [(2, 192, 1), (2, 96, 2), (2, 256, 0), (4, 64, 1), (1, 32, 0), (2, 128, 2)]:
        wins = hip.emul_attention_wins(H, dk, rel)
        assert isinstance(wins, bool)
        # default: what the precision has always meant
        assert hip.attention_dtype(hip.F32, False, None, H, dk, rel) == hip.F32
        assert hip.attention_dtype(hip.F32, True, None, H, dk, rel) == hip.F32S
        assert hip.attention_dtype(hip.F16, False, None, H, dk, rel) == hip.F16
        # "fp32" forces exact f32, "fp32_bf16x3" takes the emulated kernel exactly where the rule says so and exact f32 elsewhere
        assert hip.attention_dtype(hip.F32, True, "fp32", H, dk, rel) == hip.F32
        assert hip.attention_dtype(hip.F32, False, "fp32_bf16x3", H, dk, rel) == (hip.F32E if wins else hip.F32)
        assert hip.attention_dtype(hip.F32, True, "fp32_bf16x3", H, dk, rel) == (hip.F32E if wins else hip.F32)
    with hip.attention_precision("fp32_bf16x3"):
        assert hip._ATTENTION[0] == "fp32_bf16x3"
        with hip.attention_precision(None):
            assert hip._ATTENTION[0] is None
        assert hip._ATTENTION[0] == "fp32_bf16x3"
    assert hip._ATTENTION[0] is None


def test_decode_cli_knows_the_attention_flag():
    from jatts_amd.bin.tts_decode import get_parser
    base = ["--csv", "a", "--stats", "b", "--token-list", "c", "--token-column", "d", "--outdir", "e", "--checkpoint", "f"]
    p = get_parser()
    assert p.parse_args(base).attention_precision is None
    assert p.parse_args(base + ["--attention-precision", "fp32_bf16x3"]).attention_precision == "fp32_bf16x3"
    assert p.parse_args(base + ["--attention-precision", "fp32"]).attention_precision == "fp32"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--attention-precision", "fp16"])
    sh = open(os.path.join(ROOT, "egs", "common", "stage4.sh")).read()
    assert '${attention_precision:+--attention-precision "${attention_precision}"}' in sh


def test_abi_version_8_everywhere(lib):
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    from jatts_amd import _abi
    assert int(re.search(r"#define JATTS_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert lib.jatts_abi_version() == 8 and _abi.ABI_VERSION == 8
