"""GPU: the tap-window hint of jatts_conv1d (jatts_conv_desc.tap_group_n) on the polyphase upsampling convs.

The emulated 16 x 16 x 32 conv lets each wave contract over the two real taps of its phase group; every other kernel ignores the hint.  On the integer
operands of tests/conv_geometry_cases.py the float64 conv_transpose1d result is the expected output to the last bit, so every case compares
(a) the hinted launch, (b) the unhinted launch and (c) that reference with torch.equal, in NaN-prefilled buffers whose slack is compared bit for bit.

Shapes: strides 2 / 8 (equal groups) and 5 / 3 (2 | 3 and 1 | 2 phases); c_in 64 / 128 (one / two chunks); c_out 32 / 64 / 128 (the group boundary on wave
spans of 32 and 64), 48 (group boundaries of 48 / 96 / 192: the 384-wide tile's 48-channel wave span keeps the hint, under variant 6 and -- n_out = 384 at
s = 8 -- with the boundary inside one workgroup) and 40 (a boundary no tile's span divides: the hint is dropped); len_mul 1 / 8; one plain input, the LeakyReLU prologue, three summed
inputs with and without it; a ragged batch [70, 1, 65, 2, 64, 63]; both emulated arithmetics; every tile jatts_conv_desc.variant can force.  One further case
(s = 3, c_out = 256 at len_mul 24) is a launch the 384-wide tile takes unhinted and the 256-wide tile hinted (256 is no multiple of its 48-channel
wave span), another (s = 8, c_out = 96 at len_mul 24) one the rules give the 384-wide tile WITH its hint (boundary 384).

hinted == unhinted cannot tell a kept hint from a dropped one, so test_hint_is_kept_exactly_where_the_tile_aligns breaks the promise on purpose: with
non-zeros planted in the taps the window calls zero, a launch that keeps its hint still gives the honest weight's result, one that drops it does not."""
import collections

import pytest
import torch

import conv_geometry_cases as cg

pytestmark = pytest.mark.gpu

NAN = float("nan")
LENS = [70, 1, 65, 2, 64, 63]
STRIDES = (2, 8, 5, 3)
C_INS = (64, 128)
C_OUTS = (32, 64, 128, 48, 40)
LEN_MULS = (1, 8)
# (inputs, in_scale, LeakyReLU slope): int_operand keeps the staged operand an integer for these
OPERANDS = ((1, 1.0, None), (1, 1.0, 0.5), (3, 0.25, 0.25), (3, 0.5, None))
# 0 = the dispatcher's rules; 6 / 3 / 2 / 1 / 9 the tiles of n_out > 64 (n_out <= 64 and summed inputs have one tile each).  A number that does not apply to a
# launch falls back to the rules (and must still be right)
VARIANTS = (0, 6, 3, 2, 1, 9)
ARITHS = ("F32E", "F32E6")
Op = collections.namedtuple("Op", "n_in in_scale slope")
COL0, SLACK_ROWS = 8, 3          # the output is a window of a wider, longer NaN-prefilled buffer


def _case(s, c_in, c_out, len_mul, op):
    """Integer inputs of one polyphase launch and the float64 conv_transpose1d result as (rows, s * c_out)."""
    g = cg._gen("tapwin", s, c_in, c_out, len_mul, tuple(op))
    row_lens = [v * len_mul for v in LENS]
    xs, u = cg.int_operand((sum(row_lens), c_in), op, g)
    w = (torch.randint(-2, 3, (c_in, c_out, 2 * s), generator=g) * (torch.rand(c_in, c_out, 2 * s, generator=g) < 0.5)).float()
    b = torch.randint(-8, 9, (c_out,), generator=g).float()
    ref = cg.reference_polyphase(u, [(w, b, s)], row_lens).reshape(sum(row_lens), s * c_out)
    assert float(ref.abs().max()) < cg.F24
    return xs, w, b, ref


def _launch(hip, dev, rb, xs, wp, code, c_in, n_out, pad, bias, len_mul, op, variant, win):
    rows = rb.total * len_mul
    buf = torch.full((rows + SLACK_ROWS, COL0 + n_out + 8), NAN, dtype=torch.float32, device=dev)
    y = hip.conv1d(rb, xs, wp, c_in, n_out, 3, dtype=code, w_layout=1, pad=pad, bias=bias, pre_lrelu=op.slope, in_scale=op.in_scale, len_mul=len_mul,
                   out=buf, out_ld=buf.shape[1], out_col0=COL0, variant=variant, tap_window=win)
    assert y is buf
    return buf


def _check(buf, unhinted, ref_dev, what):
    """hinted == unhinted == reference inside the window (torch.equal), and not one bit of the NaN slack touched."""
    rows, n_out = ref_dev.shape
    win = buf[:rows, COL0:COL0 + n_out]
    assert torch.equal(win, unhinted[:rows, COL0:COL0 + n_out]), f"{what}: hinted != unhinted"
    assert torch.equal(win, ref_dev), f"{what}: hinted != float64 conv_transpose1d"
    a, b = buf.clone(), unhinted.clone()
    a[:rows, COL0:COL0 + n_out] = 0
    b[:rows, COL0:COL0 + n_out] = 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isnan(a[rows:]).all()) and bool(torch.isnan(a[:, :COL0]).all()) \
        and bool(torch.isnan(a[:, COL0 + n_out:]).all()), f"{what}: stores outside the output window"


def _run_shape(hip, dev, s, c_in, c_out, len_mul, variants):
    tg = hip.convtranspose_tap_groups(2 * s, s, cg.poly_padding(s))
    win = (tg[0] * c_out,) + tg[1:]
    n_out = s * c_out
    rb = hip.RaggedBatch(LENS, dev)
    for op in (Op(*o) for o in OPERANDS):
        xs, w, b, ref = _case(s, c_in, c_out, len_mul, op)
        wc, pad = hip.convtranspose_as_conv(w, s, cg.poly_padding(s))
        assert wc.shape[-1] == 3
        hip.check_tap_window(wc, win)
        wp = hip.pack_conv_weight_bf16x3_k32(wc.to(dev), 64)
        dxs = [x.to(dev).contiguous() for x in xs]
        bias = b.repeat(s).to(dev)
        ref_dev = ref.float().to(dev)
        for arith in ARITHS:
            code = getattr(hip, arith)
            unhinted = _launch(hip, dev, rb, dxs, wp, code, c_in, n_out, pad, bias, len_mul, op, 0, None)
            for v in variants:
                hinted = _launch(hip, dev, rb, dxs, wp, code, c_in, n_out, pad, bias, len_mul, op, v, win)
                _check(hinted, unhinted, ref_dev, f"{arith} s={s} {c_in}->{c_out} len_mul={len_mul} n_in={op.n_in} slope={op.slope} variant={v}")


@pytest.mark.parametrize("c_out", C_OUTS)
@pytest.mark.parametrize("s", STRIDES)
def test_hinted_equals_unhinted_equals_conv_transpose(cuda, lib, s, c_out):
    from jatts_amd import hip
    for c_in in C_INS:
        for len_mul in LEN_MULS:
            _run_shape(hip, cuda, s, c_in, c_out, len_mul, VARIANTS)


def test_384_wide_launch_falls_back_to_the_256_wide_tile(cuda, lib):
    """n_out = 768 on 27 x 6 time tiles: unhinted the dispatcher's rules give the 384-wide tile; the group boundary 256 is no multiple of that tile's
    48-channel wave span, so the hinted launch takes the 256-wide tile (spans of 32) and keeps its window.  Forced onto the 384-wide tile (variant 6) the
    hint is dropped."""
    from jatts_amd import hip
    _run_shape(hip, cuda, 3, 64, 256, 24, (0, 6, 3))


def test_384_wide_launch_keeps_a_hint_on_a_48_channel_boundary(cuda, lib):
    """n_out = 768 on 27 x 6 time tiles with the group boundary at 384 = 8 x 48: the rules give the 384-wide tile (NF = 3, one-step ring) and it keeps the hint."""
    from jatts_amd import hip
    _run_shape(hip, cuda, 8, 64, 96, 24, (0, 6, 3))


# (s, c_out, len_mul, inputs, variant, kept): which launches keep their hint (csrc/conv1d_emul.hip: the tile's per-wave channel span divides tap_group_n)
KEPT = [
    (8, 64, 8, 1, 0, True), (8, 64, 8, 1, 3, True), (8, 64, 8, 1, 2, True), (8, 64, 8, 1, 1, True), (8, 64, 8, 1, 9, True),   # boundary 256 on spans of 32
    (8, 64, 8, 1, 6, False),          # ... forced onto spans of 48: dropped
    (2, 48, 8, 1, 6, True),           # boundary 48 on the 384-wide tile: wave 0 | wave 1
    (2, 48, 8, 1, 0, False),          # ... on spans of 32: dropped
    (8, 96, 24, 1, 0, True),          # the rules' own 384-wide launch, boundary 384
    (3, 256, 24, 1, 0, True),         # 384-wide unhinted, 256-wide (boundary 256) hinted
    (2, 32, 8, 1, 0, True),           # n_out = 64: the 64 n x 64 t tile, spans of 32
    (2, 64, 8, 3, 0, True),           # summed inputs: spans of 64, boundary 64
    (2, 32, 8, 3, 0, False),          # ... boundary 32: dropped
    (2, 40, 8, 1, 0, False),          # boundary 40: no tile
]


@pytest.mark.parametrize("s,c_out,len_mul,n_in,variant,kept", KEPT, ids=[f"s{a}c{b}m{c}i{d}v{e}-{'kept' if f else 'dropped'}" for a, b, c, d, e, f in KEPT])
def test_hint_is_kept_exactly_where_the_tile_aligns(cuda, lib, s, c_out, len_mul, n_in, variant, kept):
    """The promise broken on purpose (nothing but values depends on it): ones planted in every tap the window calls zero.  A launch that keeps the hint never
    reads them and returns the honest weight's result; a launch that dropped it returns the planted weight's."""
    from jatts_amd import hip
    c_in, n_out = 64, s * c_out
    op = Op(n_in, 1.0 if n_in == 1 else 0.5, None)
    tg = hip.convtranspose_tap_groups(2 * s, s, cg.poly_padding(s))
    win = (tg[0] * c_out,) + tg[1:]
    xs, w, b, ref = _case(s, c_in, c_out, len_mul, op)
    wc, pad = hip.convtranspose_as_conv(w, s, cg.poly_padding(s))
    bad = wc.clone()
    bad[:win[0], :, 2] = 1.0
    bad[win[0]:, :, 0] = 1.0
    with pytest.raises(ValueError, match="not zero outside"):
        hip.check_tap_window(bad, win)
    rb = hip.RaggedBatch(LENS, cuda)
    dxs = [x.to(cuda).contiguous() for x in xs]
    bias = b.repeat(s).to(cuda)
    ref_dev = ref.float().to(cuda)
    wp_bad = hip.pack_conv_weight_bf16x3_k32(bad.to(cuda), 64)
    rows = ref_dev.shape[0]
    for arith in ARITHS:
        code = getattr(hip, arith)
        every_tap = _launch(hip, cuda, rb, dxs, wp_bad, code, c_in, n_out, pad, bias, len_mul, op, 0, None)[:rows, COL0:COL0 + n_out]
        assert not torch.equal(every_tap, ref_dev)
        y = _launch(hip, cuda, rb, dxs, wp_bad, code, c_in, n_out, pad, bias, len_mul, op, variant, win)[:rows, COL0:COL0 + n_out]
        assert torch.equal(y, ref_dev if kept else every_tap), f"{arith}: the hint was {'dropped' if kept else 'kept'}"


def _generator(dev):
    from jatts_amd.synthetic import HIFIGAN_V1_22K, synth_hifigan_state
    from jatts_amd.vocoder import HiFiGANGenerator
    params = dict(HIFIGAN_V1_22K, channels=512)
    g = HiFiGANGenerator(**params)
    g.load_state_dict(synth_hifigan_state(params, seed=0))
    return g.to(dev)


def test_prepare_refuses_a_weight_that_breaks_the_promise(cuda, lib, monkeypatch):
    """The window is derived from the structure; before the generator packs a weight it checks the dense polyphase weight against it.  A polyphase weight
    with one non-zero planted in a tap the window calls zero is refused when the generator prepares."""
    from jatts_amd import hip
    g = _generator(cuda).set_precision("fp32_bf16x3")
    g._prepare()                                            # the honest weight passes
    real = hip.convtranspose_as_conv

    def planted(w, stride, padding):
        wc, pad = real(w, stride, padding)
        wc[0, 0, 2] = 1.0                                   # phase 0 lies in group A: taps {0, 1}
        return wc, pad

    monkeypatch.setattr(hip, "convtranspose_as_conv", planted)
    g.set_precision("fp32_bf16x3_6p")                       # another key: prepares again
    with pytest.raises(ValueError, match="not zero outside"):
        g._prepare()


@pytest.mark.parametrize("precision", ["fp32_bf16x3", "fp32"])
def test_generator_with_and_without_the_window(cuda, lib, precision):
    """HiFi-GAN v1, 2 utterances x 9 frames: the waveform with the windows passed equals the waveform with them cleared."""
    from jatts_amd import hip
    g = _generator(cuda).set_precision(precision)
    mel = torch.randn(18, 80, generator=torch.Generator().manual_seed(5)).to(cuda)
    rb = hip.RaggedBatch([9, 9], cuda)
    P = g._prepare()
    wins = [u[4] for u in P["ups"]]
    assert wins == [(4 * 256, 0, 1, 2), (4 * 128, 0, 1, 2), (64, 0, 1, 2), (32, 0, 1, 2)]
    y = g.inference_batch(rb, mel).clone()
    P["ups"] = [u[:4] + (None,) for u in P["ups"]]
    assert g._prepare() is P
    y0 = g.inference_batch(rb, mel)
    assert y.numel() == 18 * g.hop and bool(torch.isfinite(y).all())
    assert torch.equal(y, y0)
