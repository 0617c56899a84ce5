"""CPU: the precision record (jatts_amd/precision.py), the operand context and hip.f32_operand built on it, the one fallback rule of the
split / emulated convs, and the prepare lifecycle the four inference classes share (jatts_amd/models/_prepared.py).  No GPU is touched."""
import pytest
import torch

from test_attn_precision_cpu import _models

NAMES = ["fp16", "fp32", "fp32_split", "fp32_bf16x3", "fp32_bf16x3_6p"]


def test_the_precision_table_literally():
    from jatts_amd import hip, precision
    from jatts_amd._abi import F16, F32, F32E, F32E6, F32S
    want = {"fp16": (F16, F16), "fp32": (F32, F32), "fp32_split": (F32, F32S), "fp32_bf16x3": (F32, F32E), "fp32_bf16x3_6p": (F32, F32E6)}
    assert {n: (r.tensors, r.operand) for n, r in precision.TABLE.items()} == want
    assert hip.PRECISIONS == ("fp16", "fp32", "fp32_split", "fp32_bf16x3", "fp32_bf16x3_6p") == precision.PRECISIONS
    assert [n for n in NAMES if precision.TABLE[n].split] == ["fp32_split"]
    assert [n for n in NAMES if precision.TABLE[n].emul] == ["fp32_bf16x3", "fp32_bf16x3_6p"]
    assert sorted(hip.ATTENTION_F32_PRECISIONS) == sorted(n for n in NAMES if want[n][0] == F32)
    with pytest.raises(AttributeError):
        precision.TABLE["fp32"].operand = F32S       # frozen
    with pytest.raises(ValueError):
        precision.record("nope")


def test_operand_context_nests_and_restores():
    from jatts_amd import hip, precision
    assert hip.operand_code() == hip.F32
    with hip.operands("fp32_bf16x3"):
        assert hip.operand_code() == hip.F32E
        with hip.operands(None):                                  # None: exact f32
            assert hip.operand_code() == hip.F32
            with hip.operands(precision.TABLE["fp32_split"]):     # a record
                assert hip.operand_code() == hip.F32S
            assert hip.operand_code() == hip.F32
        assert hip.operand_code() == hip.F32E
        with pytest.raises(RuntimeError):
            with hip.operands("fp32_bf16x3_6p"):
                assert hip.operand_code() == hip.F32E6
                raise RuntimeError("inside")
        assert hip.operand_code() == hip.F32E                     # restored on an exception too
        with pytest.raises(ValueError):
            with hip.operands("nope"):
                pass
        assert hip.operand_code() == hip.F32E
    assert hip.operand_code() == hip.F32


def test_f32_operand_under_every_precision():
    from jatts_amd import hip
    w = torch.randn(32, 64, 3, generator=torch.Generator().manual_seed(0))
    for name in ("fp16", "fp32"):
        with hip.operands(name):
            got = hip.f32_operand(w, 64)
        assert isinstance(got, torch.Tensor) and torch.equal(got, hip.pack_conv_weight(w, hip.F32, 64)), name
    with hip.operands("fp32_split"):
        got = hip.f32_operand(w, 64)
    packed, inv = hip.pack_conv_weight_split(w, 64)
    assert type(got) is hip.SplitWeight and torch.equal(got.packed, packed) and torch.equal(got.inv, inv)
    assert got.code == hip.F32S and got.layout == 0
    for name, code in (("fp32_bf16x3", hip.F32E), ("fp32_bf16x3_6p", hip.F32E6)):
        with hip.operands(name):
            got, got32 = hip.f32_operand(w, 64), hip.f32_operand(w, 32)
        assert type(got) is hip.EmulWeight and got.code == code and got.layout == 1 and got.inv is None, name
        assert torch.equal(got.packed, hip.pack_conv_weight_bf16x3_k32(w, 64)), name
        assert type(got32) is hip.EmulWeight and got32.code == code and got32.layout == 0, name
        assert torch.equal(got32.packed, hip.pack_conv_weight_bf16x3(w, 32)), name
        # the explicit-code sibling, and the lazy exact-f32 copy both prepared weights share
        assert torch.equal(hip.operand(code, w, 64).packed, got.packed)
        assert torch.equal(got.f32(), hip.pack_conv_weight(w, hip.F32, 64)) and got.f32() is got.f32()
    assert torch.equal(hip.operand(hip.F16, w, 64), hip.pack_conv_weight(w, hip.F16, 64))


def test_fallback_rule_at_its_edge():
    from jatts_amd import hip
    for k_w, dil in ((3, 16), (33, 1)):
        assert hip.conv_halo_fits(k_w, dil), (k_w, dil)
    for k_w, dil in ((3, 17), (12, 3), (34, 1)):
        assert not hip.conv_halo_fits(k_w, dil), (k_w, dil)


GPU_ONLY = {     # the parent's messages, character for character
    "FastSpeech2": "jatts_amd.FastSpeech2 runs on the GPU only (no CPU fallback); call .to('cuda')",
    "VITS": "jatts_amd.VITS runs on the GPU only (no CPU fallback); call .to('cuda')",
    "MatchaTTS": "jatts_amd Matcha-TTS runs on the GPU only (no CPU fallback); call .to('cuda')",
    "MatchaTTS_MAS": "jatts_amd Matcha-TTS runs on the GPU only (no CPU fallback); call .to('cuda')",
    "HiFiGANGenerator": "jatts_amd HiFiGANGenerator runs on the GPU only (no CPU fallback)",
}


def _vocoder(**kw):
    from jatts_amd.vocoder import HiFiGANGenerator
    return HiFiGANGenerator(**dict(dict(channels=64, upsample_scales=(2,), upsample_kernel_sizes=(4,), resblock_kernel_sizes=(3,),
                                        resblock_dilations=((1,),)), **kw))


def test_prepare_lifecycle_of_all_four_classes(golden_dir):
    from jatts_amd._abi import JattsHipError
    sentinel = {"key": "sentinel"}
    for m in _models(golden_dir) + [_vocoder()]:
        name = type(m).__name__
        acoustic = name != "HiFiGANGenerator"
        assert m.precision == "fp32" and m._prep is None, name
        assert m.set_precision("fp32_bf16x3") is m
        m._prep = dict(sentinel)
        m.set_precision("fp32_bf16x3")
        assert m._prep == sentinel, f"{name}: the same precision keeps the prepared state"
        m.set_precision("fp32_split")
        assert m._prep is None and m.precision == "fp32_split", f"{name}: another precision clears it"
        if acoustic:
            m._prep = dict(sentinel)
            m.set_precision("fp32_split", attention="fp32")
            assert m._prep is None and m.attention == "fp32", f"{name}: another attention clears it"
            with pytest.raises(ValueError):
                m.set_precision("fp16", attention="fp32_bf16x3")
        m._prep = dict(sentinel)
        m.load_state_dict(m.state_dict())
        assert m._prep is None, f"{name}: load_state_dict clears it"
        m._prep = dict(sentinel)
        m.float()
        assert m._prep is None, f"{name}: _apply clears it"
        prec, att = m.precision, m.attention
        with pytest.raises(ValueError):
            m.set_precision("nope")
        assert (m.precision, m.attention) == (prec, att)
        with pytest.raises(JattsHipError) as e:
            m._prepare()
        assert str(e.value) == GPU_ONLY[name]
        if acoustic:      # train(True) turns requires_grad on; eval() leaves it
            assert not any(p.requires_grad for p in m.parameters())
            m.train()
            assert all(p.requires_grad for p in m.parameters()) and m.training
            m.eval()
    with pytest.raises(NotImplementedError):
        _vocoder(use_additional_convs=False).set_precision("fp32_split")
    with pytest.raises(TypeError):
        _vocoder().set_precision("fp32", attention="fp32")       # the vocoder has no attention switch
