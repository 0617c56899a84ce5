"""GPU parity: HiFiGANGenerator without the additional convs (HiFi-GAN V3: single-conv dilation units, csrc/resunit1_*) and with bias=False, against the
CPU oracle's no-convs2 path (oracle/hifigan_oracle.py; pinned on plain torch.nn modules by tests/test_hifigan_variants_cpu.py).

Tolerances are those of tests/test_hifigan_gpu.py: max|y - oracle| <= 2e-4 for the f32-class precisions, 2e-2 for fp16, and for the f32-class ones also
<= 5e-6 against the oracle run in float64 (the f32 CPU oracle itself sits at 7.4e-7 from it on the V3 case; outputs are unsaturated: max |y| 0.80).
"""
import functools

import numpy as np
import pytest
import torch

from helpers import maxdiff
from jatts_amd.synthetic import HIFIGAN_V1_22K, HIFIGAN_V3_22K, synth_hifigan_state

pytestmark = pytest.mark.gpu

PARAMS = {
    "v3": HIFIGAN_V3_22K,
    "v3-nobias": dict(HIFIGAN_V3_22K, bias=False),
    "v1-128-single-conv": dict(HIFIGAN_V1_22K, channels=128, use_additional_convs=False),      # V1 kernels / dilations, 16- and 8-channel stages padded to 32
    "v3-two-blocks": dict(HIFIGAN_V3_22K, resblock_kernel_sizes=(3, 5), resblock_dilations=((1, 2), (2, 6, 3))),     # MRF over two blocks
}
LENS = [21, 8]
PRECISIONS = [("fp32", 2e-4), ("fp32_bf16x3", 2e-4), ("fp32_bf16x3_6p", 2e-4), ("fp16", 2e-2)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """state, mels, the f32 oracle's and the float64 oracle's waveforms per utterance (computed once, shared, left unchanged)."""
    from oracle.hifigan_oracle import hifigan_generate
    params = PARAMS[name]
    sd = synth_hifigan_state(params, seed=3)
    gen = torch.Generator().manual_seed(0)
    mels = [torch.randn(n, 80, generator=gen) for n in LENS]
    sd64 = {k: v.double() for k, v in sd.items()}
    ref32 = [hifigan_generate(sd, c, params["upsample_scales"], params["resblock_dilations"]) for c in mels]
    ref64 = [hifigan_generate(sd64, c.double(), params["upsample_scales"], params["resblock_dilations"]) for c in mels]
    return sd, mels, ref32, ref64


@pytest.mark.parametrize("prec,tol", PRECISIONS)
@pytest.mark.parametrize("name", list(PARAMS))
def test_generator_without_additional_convs_matches_oracle(cuda, lib, name, prec, tol):
    from jatts_amd import hip
    from jatts_amd.vocoder import HiFiGANGenerator
    params = PARAMS[name]
    sd, mels, ref32, ref64 = _case(name)
    g = HiFiGANGenerator(**params)
    g.load_state_dict(sd)
    g = g.to(cuda).set_precision(prec)
    hop = g.hop
    assert hop == 256
    rb = hip.RaggedBatch(LENS, cuda)
    y = g.inference_batch(rb, torch.cat(mels).to(cuda))
    assert y.shape == (sum(LENS) * hop,)
    o = 0
    for n, r32, r64 in zip(LENS, ref32, ref64):
        got = y[o * hop:(o + n) * hop]
        e, e64 = maxdiff(got, r32), maxdiff(got, r64)
        print(f"{name} {prec} T={n}: max|y - oracle f32| {e:.3e}, max|y - oracle f64| {e64:.3e}, max|y| {float(got.abs().max()):.3f}")
        assert e <= tol, f"{name} {prec}: max|d| = {e:.3e}"
        if prec != "fp16":
            assert e64 <= 5e-6, f"{name} {prec}: max|d| against float64 = {e64:.3e}"
        assert float(got.abs().max()) <= 1.0
        o += n
    # the single-utterance API: (T * hop, 1), equal to the batch slice; first sight eager, then captured, then replayed -- bit-identical
    y1 = g.inference(mels[1])
    assert y1.shape == (LENS[1] * hop, 1)
    assert maxdiff(y1.view(-1), y[LENS[0] * hop:]) <= 1e-6
    y2 = g.inference(mels[1])
    y3 = g.inference(mels[1])
    assert torch.equal(y1, y2) and torch.equal(y1, y3)


def test_single_conv_generators_never_take_the_fused_resblock_route(cuda, lib, monkeypatch):
    """The fused whole-ResBlock launches are two-conv kernels: a generator without the additional convs issues single-conv units only, every one with
    w2 = b2 = None."""
    from jatts_amd import hip
    from jatts_amd.vocoder import HiFiGANGenerator
    sd, mels, _, _ = _case("v3")
    g = HiFiGANGenerator(**HIFIGAN_V3_22K)
    g.load_state_dict(sd)
    g = g.to(cuda).set_precision("fp16")        # (fp16 fuses the most two-conv shapes: (32, 3), (32, 7), (64, 3))
    seen = []
    real = hip.hifigan_resunit

    def unit(rb, len_mul, x, y, w1, b1, w2, b2, *a, **k):
        seen.append((w2, b2, a[0], a[1], a[2], len(k.get("add") or ())))
        return real(rb, len_mul, x, y, w1, b1, w2, b2, *a, **k)

    def block(*a, **k):
        raise AssertionError("hifigan_resblock launched for a generator without additional convs")

    monkeypatch.setattr(hip, "hifigan_resunit", unit)
    monkeypatch.setattr(hip, "hifigan_resblock", block)
    g.inference_batch(hip.RaggedBatch(LENS, cuda), torch.cat(mels).to(cuda))
    assert len(seen) == 3 * 3 * 2 and all(w2 is None and b2 is None for w2, b2, *_ in seen)
    assert [(c, k, d) for _, _, c, k, d, _ in seen[:6]] == [(128, 3, 1), (128, 3, 2), (128, 5, 2), (128, 5, 6), (128, 7, 3), (128, 7, 12)]
    # the MRF mean rides in the last unit of the last ResBlock of every stage
    assert [n for *_, n in seen] == [0, 0, 0, 0, 0, 2] * 3


def test_vocoder_decodes_a_v3_config(cuda, lib):
    from jatts_amd.vocoder import Vocoder
    sd, _, _, _ = _case("v3")
    rng = np.random.default_rng(0)
    stats = {"mean": rng.normal(size=80).astype(np.float32), "scale": (0.5 + rng.random(80)).astype(np.float32)}
    trg = {"mean": rng.normal(size=80).astype(np.float32), "scale": (0.5 + rng.random(80)).astype(np.float32)}
    voc = Vocoder(sd, {"sampling_rate": 22050, "generator_type": "HiFiGANGenerator", "generator_params": HIFIGAN_V3_22K}, stats, cuda, trg_stats=trg)
    c = torch.randn(17, 80, generator=torch.Generator().manual_seed(1)).to(cuda)
    y, sr = voc.decode(c)
    assert sr == 22050 and y.dim() == 1 and y.numel() == c.shape[0] * 256 and y.is_cuda
    want = voc.model.inference(voc.normalized(c)).view(-1)
    assert maxdiff(y, want) <= 1e-6
    assert float(y.abs().max()) > 0.01


def test_fp32_split_refused_on_the_device_too(cuda, lib):
    from jatts_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(**HIFIGAN_V3_22K).to(cuda)
    with pytest.raises(NotImplementedError, match="fp32_split"):
        g.set_precision("fp32_split")
    assert g.precision == "fp32"
