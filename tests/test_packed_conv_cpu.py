"""CPU: hip.PackedConv, the prepared Conv1d / Linear layer the inference models launch by calling it -- its fields against the formulas written out
here on the raw tensors, its operand under every precision, and what a call refuses.  Nothing is launched."""
import pytest
import torch

from jatts_amd import _abi, hip, precision

CPU = torch.device("cpu")
PRECISIONS = ["fp16", "fp32", "fp32_split", "fp32_bf16x3", "fp32_bf16x3_6p"]


def _raw(kind, fold):
    g = torch.Generator().manual_seed(11)
    w = torch.randn((32, 48, 3) if kind == "conv" else (32, 48), generator=g)
    b = torch.randn(32, generator=g)
    scale, shift = (torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)) if fold else (None, None)
    return w, b, scale, shift


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "scale-shift"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_fields_are_the_constructor_formulas(lib, kind, with_bias, fold):
    w, b, scale, shift = _raw(kind, fold)
    pc = hip.PackedConv(w, b if with_bias else None, hip.F32, CPU, scale=scale, shift=shift)
    w3 = w if w.dim() == 3 else w.unsqueeze(-1)            # a Linear is a k = 1 conv
    want_b = b if with_bias else None
    if fold:                                                # y = (W x + b) * scale + shift, per output channel
        w3 = w3 * scale.view(-1, 1, 1)
        want_b = (b * scale if with_bias else torch.zeros(32)) + shift
    assert (pc.n_out, pc.k, pc.c_in, pc.dtype) == (32, 3 if kind == "conv" else 1, 64, hip.F32)
    assert (pc.b is None) == (want_b is None)
    if want_b is not None:
        assert pc.b.dtype == torch.float32 and pc.b.is_contiguous() and torch.equal(pc.b, want_b)
    assert isinstance(pc.w, torch.Tensor) and torch.equal(pc.w, hip.pack_conv_weight(w3, hip.F32, 64))
    assert pc.w.numel() == 32 * 64 * pc.k                   # n_out rounded up to 32, c_in to 64: what conv1d checks against n_out / c_in / k_w


@pytest.mark.parametrize("kind", ["conv", "linear"])
@pytest.mark.parametrize("name", PRECISIONS)
def test_operand_is_f32_operands_under_every_precision(lib, name, kind):
    w, b, _, _ = _raw(kind, False)
    w3 = w if w.dim() == 3 else w.unsqueeze(-1)
    rec = precision.record(name)
    with hip.operands(name):
        pc = hip.PackedConv(w, b, hip.F32, CPU)
        want = hip.f32_operand(w3, 64)
        pt = hip.PackedConv(w, b, rec.tensors, CPU)         # as a model prepares it: the precision's tensor dtype
    assert hip.operand_code() == hip.F32                    # (the context is closed again)
    assert pc.dtype == hip.F32 and pt.dtype == rec.tensors
    if name in ("fp16", "fp32"):                            # packed exact f32; f16 tensors take the f16 packing
        assert isinstance(pc.w, torch.Tensor) and pc.w.dtype == torch.float32 and torch.equal(pc.w, want)
        assert isinstance(pt.w, torch.Tensor) and torch.equal(pt.w, hip.pack_conv_weight(w3, rec.tensors, 64))
        return
    assert type(pc.w) is type(want) and isinstance(pc.w, hip.PreparedWeight) and type(pt.w) is type(want)
    code, layout = {"fp32_split": (hip.F32S, 0), "fp32_bf16x3": (hip.F32E, 1), "fp32_bf16x3_6p": (hip.F32E6, 1)}[name]
    assert (pc.w.code, pc.w.layout) == (code, layout) == (rec.operand, want.layout)
    assert torch.equal(pc.w.packed, want.packed) and torch.equal(pt.w.packed, want.packed)
    assert (pc.w.inv is None) == (name != "fp32_split") and (pc.w.inv is None or torch.equal(pc.w.inv, want.inv))
    assert torch.equal(pc.w.f32(), hip.pack_conv_weight(w3, hip.F32, 64))       # the fallback operand of a halo that does not fit


def test_a_call_refuses_cpu_tensors_and_the_records_own_fields(lib):
    w, b, _, _ = _raw("conv", False)
    pc = hip.PackedConv(w, b, hip.F32, CPU)
    rb = hip.RaggedBatch([1, 40], CPU)
    x = torch.zeros(41, 64)
    with pytest.raises(_abi.JattsHipError, match="no CPU fallback"):
        pc(rb, x)
    with pytest.raises(_abi.JattsHipError, match="no CPU fallback"):
        pc(rb, x, bias=None, act=hip.ACT_RELU)
    for kw in (dict(dtype=hip.F32), dict(n_out=8), dict(c_in=64), dict(k_w=3), dict(w_packed=pc.w)):
        with pytest.raises(TypeError):
            pc(rb, x, **kw)
