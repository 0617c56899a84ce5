"""GPU: the single prepared-weight branch of hip.conv1d at the edge of its fallback rule, and the vocoder's single unit-conv class in every
precision.  Shape checks of the Python routing (bit-equality with the explicit launch each wrapper stands for); the numerical pins of these
kernels are tests/test_emul_gpu.py, test_kernels_gpu.py and test_hifigan*_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp16", "fp32", "fp32_split", "fp32_bf16x3", "fp32_bf16x3_6p"]


@pytest.mark.parametrize("kind", ["split", "emul7", "emul6"])
@pytest.mark.parametrize("dil", [16, 17], ids=["halo32-fits", "halo34-falls-back"])
def test_prepared_weight_is_the_explicit_launch(cuda, lib, kind, dil):
    from jatts_amd import hip
    c_in, n_out, k_w, lens = 64, 32, 3, [1, 40]
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(n_out, c_in, k_w, generator=g) / (c_in * k_w) ** 0.5).to(cuda)
    x = torch.randn(sum(lens), c_in, generator=g).to(cuda)
    b = torch.randn(n_out, generator=g).to(cuda)
    rb = hip.RaggedBatch(lens, cuda)
    prepared = hip.SplitWeight(w, 64) if kind == "split" else hip.EmulWeight(w, 64, hip.F32E if kind == "emul7" else hip.F32E6)
    assert (prepared.code, prepared.layout, prepared.inv is None) == {"split": (hip.F32S, 0, False), "emul7": (hip.F32E, 1, True),
                                                                      "emul6": (hip.F32E6, 1, True)}[kind]
    y = hip.conv1d(rb, x, prepared, c_in, n_out, k_w, dtype=hip.F32, dil=dil, bias=b)
    if dil == 16:       # the last halo that fits: the packed operand with its dtype code, inverse scales and layout spelled out
        ref = hip.conv1d(rb, x, prepared.packed, c_in, n_out, k_w, dtype=prepared.code, dil=dil, bias=b, w_inv=prepared.inv,
                         w_layout=prepared.layout, out_f32=True)
    else:               # the first that does not: the exact-f32 kernel on the same weight
        ref = hip.conv1d(rb, x, hip.pack_conv_weight(w, hip.F32, 64), c_in, n_out, k_w, dtype=hip.F32, dil=dil, bias=b)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and y.shape == (sum(lens), n_out) and torch.isfinite(y).all()
    assert torch.equal(y, ref)


@pytest.mark.parametrize("prec,additional", [(p, True) for p in PRECISIONS] + [(p, False) for p in PRECISIONS if p != "fp32_split"],
                         ids=lambda v: v if isinstance(v, str) else "two-conv-units" if v else "single-conv-units")
def test_vocoder_unit_convs_in_every_precision(cuda, lib, prec, additional):
    """(fp32_split has no single-conv unit: set_precision refuses it, tests/test_precision_cpu.py.)"""
    from jatts_amd import hip
    from jatts_amd.synthetic import synth_hifigan_state
    from jatts_amd.vocoder import HiFiGANGenerator
    params = dict(in_channels=80, out_channels=1, channels=64, kernel_size=7, upsample_scales=(2,), upsample_kernel_sizes=(4,),
                  resblock_kernel_sizes=(3, 7), resblock_dilations=((1, 3), (1, 3)), use_additional_convs=additional)
    g = HiFiGANGenerator(**params)
    g.load_state_dict(synth_hifigan_state(params, seed=2))
    g = g.to(cuda).set_precision(prec)
    lens = [3, 9]
    mel = torch.randn(sum(lens), 80, generator=torch.Generator().manual_seed(1)).to(cuda)
    y1 = g.inference_batch(hip.RaggedBatch(lens, cuda), mel)
    y2 = g.inference_batch(hip.RaggedBatch(lens, cuda), mel)
    torch.cuda.synchronize()
    assert y1.shape == (sum(lens) * g.hop,) and torch.isfinite(y1).all() and torch.equal(y1, y2)
    convs = [c for stage in g._prep["blocks"] for units in stage for c1, c2, _, _ in units for c in (c1, c2)]
    assert len(convs) == 2 * 2 * 2 and all((c is None) == (not additional) for c in convs[1::2])
    for c in convs:
        if c is None:        # (the second conv of a single-conv unit)
            continue
        assert c.w is not None and c.b is not None and c.w_block is not None
        assert (c.inv is not None) == (prec == "fp32_split")
        assert c.layout == (1 if prec in ("fp32_bf16x3", "fp32_bf16x3_6p") else 0)
