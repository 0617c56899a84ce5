"""CPU: HiFiGANGenerator configurations beyond V1 -- use_additional_convs=False (HiFi-GAN V3: single-conv dilation units) and bias=False --
construct, expose the state_dict schema of the synthetic states and load them; and the CPU oracle's no-convs2 path (the yardstick of
tests/test_hifigan_variants_gpu.py) equals a generator composed here from plain torch.nn modules, in float64."""
import pytest
import torch

from jatts_amd.synthetic import HIFIGAN_V1_22K, HIFIGAN_V3_22K, synth_hifigan_state

V3_NOBIAS = dict(HIFIGAN_V3_22K, bias=False)


def test_v3_params_are_the_published_configuration():
    p = HIFIGAN_V3_22K
    assert p["channels"] == 256 and p["upsample_scales"] == (8, 8, 4) and p["upsample_kernel_sizes"] == (16, 16, 8)
    assert p["resblock_kernel_sizes"] == (3, 5, 7) and p["resblock_dilations"] == ((1, 2), (2, 6), (3, 12))
    assert p["use_additional_convs"] is False and p["bias"] is True
    assert {k: v for k, v in p.items() if k not in ("channels", "upsample_scales", "upsample_kernel_sizes", "resblock_kernel_sizes", "resblock_dilations",
                                                    "use_additional_convs")} == \
           {k: v for k, v in HIFIGAN_V1_22K.items() if k not in ("channels", "upsample_scales", "upsample_kernel_sizes", "resblock_kernel_sizes",
                                                                 "resblock_dilations", "use_additional_convs")}


@pytest.mark.parametrize("params", [HIFIGAN_V3_22K, V3_NOBIAS, dict(HIFIGAN_V1_22K, channels=128, use_additional_convs=False),
                                    dict(HIFIGAN_V1_22K, channels=128, bias=False)], ids=["v3", "v3-nobias", "v1-single-conv", "v1-nobias"])
def test_constructor_and_schema(params):
    """The constructor accepts the configuration (it raised NotImplementedError before), the module's keys are exactly the synthetic state's -- no convs2
    without the additional convs, no upsample / ResBlock bias with bias=False -- and the state loads."""
    from jatts_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(**params)
    sd = synth_hifigan_state(params, seed=3)
    keys = set(g.state_dict().keys())
    assert keys == set(sd.keys())
    if not params["use_additional_convs"]:
        assert not any(".convs2." in k for k in keys)
    if not params["bias"]:
        assert not any(k.endswith(".bias") and (k.startswith("upsamples.") or k.startswith("blocks.")) for k in keys)
        assert "input_conv.bias" in keys and "output_conv.1.bias" in keys
    assert any(".convs1." in k for k in keys)
    for k, v in g.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape), k
    g.load_state_dict(sd)
    for k, v in g.state_dict().items():
        assert torch.equal(v, sd[k]), k
    hop = 1
    for s in params["upsample_scales"]:
        hop *= s
    assert g.hop == hop == 256


def test_existing_states_are_unchanged_by_the_bias_switch():
    """synth_hifigan_state is additive: every tensor has its own named generator, so a V1 state's tensors do not depend on keys another configuration omits."""
    a = synth_hifigan_state(dict(HIFIGAN_V1_22K, channels=64), seed=3)
    b = synth_hifigan_state(dict(HIFIGAN_V1_22K, channels=64, bias=False), seed=3)
    c = synth_hifigan_state(dict(HIFIGAN_V1_22K, channels=64, use_additional_convs=False), seed=3)
    for other in (b, c):
        assert set(other) < set(a)
        for k, v in other.items():
            assert torch.equal(v, a[k]), k


def test_fp32_split_is_refused_without_additional_convs():
    from jatts_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(**HIFIGAN_V3_22K)
    with pytest.raises(NotImplementedError, match="fp32_split"):
        g.set_precision("fp32_split")
    for prec in ("fp32", "fp16", "fp32_bf16x3", "fp32_bf16x3_6p"):
        assert g.set_precision(prec).precision == prec
    assert HiFiGANGenerator(**dict(HIFIGAN_V1_22K, channels=64)).set_precision("fp32_split").precision == "fp32_split"


class _TorchV3(torch.nn.Module):
    """The generator without additional convs from plain torch.nn modules, in parallel_wavegan's module layout (the keys of oracle/hifigan_oracle.py's header)."""

    def __init__(self, p):
        super().__init__()
        nn = torch.nn
        ch, k, bias = p["channels"], p["kernel_size"], p["bias"]
        slope = p["nonlinear_activation_params"]["negative_slope"]
        self.input_conv = nn.Conv1d(p["in_channels"], ch, k, padding=(k - 1) // 2)
        self.upsamples, self.blocks = nn.ModuleList(), nn.ModuleList()
        self.nb = len(p["resblock_kernel_sizes"])
        c = ch
        for s, uk in zip(p["upsample_scales"], p["upsample_kernel_sizes"]):
            self.upsamples.append(nn.Sequential(nn.LeakyReLU(slope), nn.ConvTranspose1d(c, c // 2, uk, s, padding=s // 2 + s % 2, output_padding=s % 2, bias=bias)))
            c //= 2
            for rk, dils in zip(p["resblock_kernel_sizes"], p["resblock_dilations"]):
                blk = nn.Module()
                blk.convs1 = nn.ModuleList(nn.Sequential(nn.LeakyReLU(slope), nn.Conv1d(c, c, rk, dilation=d, padding=(rk - 1) // 2 * d, bias=bias)) for d in dils)
                self.blocks.append(blk)
        self.output_conv = nn.Sequential(nn.LeakyReLU(), nn.Conv1d(c, p["out_channels"], k, padding=(k - 1) // 2), nn.Tanh())

    def forward(self, c):
        x = self.input_conv(c.t().unsqueeze(0))
        for i, up in enumerate(self.upsamples):
            x = up(x)
            cs = 0.0
            for j in range(self.nb):
                y = x
                for unit in self.blocks[i * self.nb + j].convs1:
                    y = unit(y) + y
                cs = cs + y
            x = cs / self.nb
        return self.output_conv(x).reshape(-1)


@pytest.mark.parametrize("bias", [True, False])
def test_oracle_no_convs2_path_equals_plain_torch_modules(bias):
    """The yardstick of the GPU tests: oracle.hifigan_oracle.hifigan_generate on a float64 V3 state against torch.nn.Conv1d / ConvTranspose1d / LeakyReLU
    modules loaded with the same tensors (strict=True).  13 frames; float64 on both sides: <= 1e-12 (0.0 where this was written)."""
    from oracle.hifigan_oracle import hifigan_generate
    p = dict(HIFIGAN_V3_22K, bias=bias)
    sd = {k: v.double() for k, v in synth_hifigan_state(p, seed=3).items()}
    m = _TorchV3(p).double()
    m.load_state_dict(sd, strict=True)
    mel = torch.randn(13, 80, generator=torch.Generator().manual_seed(0)).double()
    with torch.no_grad():
        want = m(mel)
        got = hifigan_generate(sd, mel, p["upsample_scales"], p["resblock_dilations"])
    assert got.shape == want.shape == (13 * 256,)
    assert float(got.abs().max()) > 0.05          # a live signal, not zeros
    e = float((got - want).abs().max())
    assert e <= 1e-12, e


def test_library_marks_the_single_conv_unit(lib):
    """jatts_resunit_single_conv: bound at load (a library from before the single-conv unit lacks the symbol and is refused there, the ABI number
    being unchanged) and 1 exactly for the arithmetics that have a kernel."""
    from jatts_amd import _abi, hip
    assert "jatts_resunit_single_conv" in _abi.PROTOTYPES
    ok = {(hip.F32, 0), (hip.F16, 0), (hip.F32E, 1), (hip.F32E6, 1)}
    for code in (hip.F32, hip.F16, hip.F32S, hip.F32E, hip.F32E6):
        for layout in (0, 1):
            assert lib.jatts_resunit_single_conv(code, layout) == int((code, layout) in ok), (code, layout)
