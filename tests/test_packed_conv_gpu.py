"""GPU: calling a hip.PackedConv is bit for bit the explicit hip.conv1d launch with every field of the record spelled out -- under each of the
five precisions, with the epilogue keywords the models use, without a bias, past the halo the split / emulated kernels cover, and for the
two-output Q | K | V projection."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp16", "fp32", "fp32_split", "fp32_bf16x3", "fp32_bf16x3_6p"]
LENS = [1, 40]


def _layer(hip, cuda, prec, c, n_out=32, k=3, seed=5):
    """-> (PackedConv prepared as a model does under `prec`, the raw f32 weight on the device, input of the packed width in the tensor dtype)."""
    from jatts_amd import precision
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(n_out, c, k, generator=g) / (c * k) ** 0.5).to(cuda)
    b = torch.randn(n_out, generator=g).to(cuda)
    dt = precision.record(prec).tensors
    with hip.operands(prec):
        pc = hip.PackedConv(w, b, dt, cuda)
    x = torch.zeros(sum(LENS), pc.c_in)
    x[:, :c] = torch.randn(sum(LENS), c, generator=g)
    return pc, w, x.to(cuda).to(hip.torch_dtype(dt))


def _explicit(hip, rb, x, pc, w, dil=1, **kw):
    """The launch pc(rb, x, dil=dil, **kw) stands for, every field spelled out (tests/test_precision_gpu.py::test_prepared_weight_is_the_explicit_launch)."""
    n_out, c, k = w.shape
    c_pad = hip.round_up(c, 64)
    if not isinstance(pc.w, hip.PreparedWeight):            # fp16 / fp32: the packed tensor of the tensor dtype
        return hip.conv1d(rb, x, hip.pack_conv_weight(w, pc.dtype, 64), c_pad, n_out, k, dtype=pc.dtype, dil=dil, **kw)
    if hip.conv_halo_fits(k, dil):                          # the packed operand with its dtype code, inverse scales and layout; f32 out
        kw["out_f32"] = True
        return hip.conv1d(rb, x, pc.w.packed, c_pad, n_out, k, dtype=pc.w.code, dil=dil, w_inv=pc.w.inv, w_layout=pc.w.layout, **kw)
    return hip.conv1d(rb, x, hip.pack_conv_weight(w, hip.F32, 64), c_pad, n_out, k, dtype=hip.F32, dil=dil, **kw)   # the exact-f32 kernel on the same weight


def _same(y, ref, shape):
    torch.cuda.synchronize()
    assert y.shape == ref.shape == shape and y.dtype == ref.dtype and torch.isfinite(y).all()
    assert torch.equal(y, ref)


@pytest.mark.parametrize("c", [64, 48], ids=["c64", "c48-padded-to-64"])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_call_is_the_explicit_launch(cuda, lib, prec, c):
    from jatts_amd import hip
    pc, w, x = _layer(hip, cuda, prec, c)
    rb = hip.RaggedBatch(LENS, cuda)
    assert (pc.c_in, pc.n_out, pc.k) == (64, 32, 3)
    for act in (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_TANH):
        _same(pc(rb, x, act=act), _explicit(hip, rb, x, pc, w, bias=pc.b, act=act), (sum(LENS), 32))


@pytest.mark.parametrize("c", [64, 48], ids=["c64", "c48-padded-to-64"])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_residual_in_place_f32_output(cuda, lib, prec, c):
    from jatts_amd import hip
    pc, w, x = _layer(hip, cuda, prec, c)
    rb = hip.RaggedBatch(LENS, cuda)
    h0 = torch.randn(sum(LENS), 32, generator=torch.Generator().manual_seed(6)).to(cuda)
    h, href = h0.clone(), h0.clone()
    y = pc(rb, x, alpha=0.5, resid=h, out=h, out_f32=True)
    ref = _explicit(hip, rb, x, pc, w, bias=pc.b, alpha=0.5, resid=href, out=href, out_f32=True)
    assert y is h and ref is href and y.dtype == torch.float32
    _same(y, ref, (sum(LENS), 32))
    assert not torch.equal(y, h0)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_bias_none_launches_without_one(cuda, lib, prec):
    from jatts_amd import hip
    pc, w, x = _layer(hip, cuda, prec, 64)
    rb = hip.RaggedBatch(LENS, cuda)
    y = pc(rb, x, bias=None)
    _same(y, _explicit(hip, rb, x, pc, w), (sum(LENS), 32))
    assert not torch.equal(y, pc(rb, x))                    # (the record's bias is not zero)
    with hip.operands(prec):
        nb = hip.PackedConv(w, None, pc.dtype, cuda)        # a record prepared without one launches without one
    assert nb.b is None
    _same(nb(rb, x), y, (sum(LENS), 32))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_dilation_past_the_staged_halo_falls_back_to_exact_f32(cuda, lib, prec):
    from jatts_amd import hip
    pc, w, x = _layer(hip, cuda, prec, 64)
    rb = hip.RaggedBatch(LENS, cuda)
    assert not hip.conv_halo_fits(pc.k, 17)
    _same(pc(rb, x, dil=17), _explicit(hip, rb, x, pc, w, dil=17, bias=pc.b), (sum(LENS), 32))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_split_returns_the_explicit_pair(cuda, lib, prec):
    from jatts_amd import hip
    pc, w, x = _layer(hip, cuda, prec, 64, n_out=512, k=1, seed=8)
    rb = hip.RaggedBatch(LENS, cuda)
    vcol, ldvt = rb.vt_layout()
    out, out2 = pc(rb, x, split=(256, ldvt, vcol))
    ref, ref2 = _explicit(hip, rb, x, pc, w, bias=pc.b, split=(256, ldvt, vcol))
    _same(out, ref, (sum(LENS), 256))
    assert out2.shape == ref2.shape == (256, ldvt) and out2.dtype == ref2.dtype
    cols = torch.cat([torch.arange(int(c0), int(c0) + n) for c0, n in zip(vcol.tolist(), LENS)]).to(cuda)     # (the slack columns of V^T stay uninitialised)
    assert torch.isfinite(out2[:, cols]).all() and torch.equal(out2[:, cols], ref2[:, cols])
