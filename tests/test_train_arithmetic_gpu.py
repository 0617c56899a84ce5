"""GPU: autograd.Conv1dFunction under autograd.arithmetic launches exactly what the explicit calls launch -- hip.conv1d on the operand packed by the
device packers with its dtype code, inverse scales and layout spelled out, hip.conv1d_wgrad for the weight and bias gradient -- in each of the three
trainer precisions, at the last halo that fits the split / emulated kernels (dil 16: 32 rows), at the first that does not (dil 17: the exact-f32 kernel
on the same weight) and on a shape whose channels are padded both ways; and a backward that runs after the context has exited launches what its
forward decided.  Every comparison is bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [1, 40]
# (c_in, n_out, k, dil): test_prepared_weight_is_the_explicit_launch's shape at halo 32 and 34, and one with c_in and n_out both padded to 64
SHAPES = [(64, 32, 3, 16), (64, 32, 3, 17), (48, 20, 7, 3)]
SHAPE_IDS = ["halo32-fits", "halo34-falls-back", "padded-channels"]
PRECISIONS = ["fp32", "fp32_split", "fp32_bf16x3"]


def _inputs(cuda, c_in, n_out, k, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(n_out, c_in, k, generator=g) / (c_in * k) ** 0.5).to(cuda)
    x = torch.randn(sum(LENS), c_in, generator=g).to(cuda)
    b = torch.randn(n_out, generator=g).to(cuda)
    gy = torch.randn(sum(LENS), n_out, generator=g).to(cuda)
    return w, x, b, gy


def _explicit_conv(hip, rb, code, x, w, n_out, k, dil, pad, bias, dgrad):
    """hip.conv1d with everything spelled out: `code`'s device packing of w (dgrad: the data-gradient operand), the input widened to the packed c_in."""
    if code == hip.F32S:
        wp, inv, c_pad = hip.pack_conv_weight_split_dev(w, dgrad=dgrad)
        kw = dict(dtype=hip.F32S, w_inv=inv, w_layout=0)
    elif code == hip.F32E:
        wp, c_pad = hip.pack_conv_weight_bf16x3_dev(w, dgrad=dgrad)
        kw = dict(dtype=hip.F32E, w_layout=1)
    else:
        wp, c_pad = hip.pack_conv_weight_dev(w, hip.F32, dgrad=dgrad)
        kw = dict(dtype=hip.F32)
    xin = x if x.shape[1] == c_pad else hip.affine_cast(x, hip.F32, ldy=c_pad)
    return hip.conv1d(rb, xin, wp, c_pad, n_out, k, dil=dil, pad=pad, bias=bias, out_f32=True, **kw)


def _run(cuda, shape, precision, seed=5):
    from jatts_amd import hip
    from jatts_amd.autograd import Conv1dFunction, arithmetic
    c_in, n_out, k, dil = shape
    pad = (k - 1) // 2 * dil
    w, x, b, gy = _inputs(cuda, c_in, n_out, k, seed)
    rb = hip.RaggedBatch(LENS, cuda)
    xd, wd, bd = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    with arithmetic(precision):
        y = Conv1dFunction.apply(xd, wd, bd, rb, dil, pad)
        y.backward(gy)
    return hip, rb, (w, x, b, gy), pad, (y.detach(), xd.grad, wd.grad, bd.grad)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_conv1d_function_is_the_explicit_launch(cuda, lib, shape, precision):
    from jatts_amd.precision import train_arithmetic
    c_in, n_out, k, dil = shape
    hip, rb, (w, x, b, gy), pad, (y, dx, dw, db) = _run(cuda, shape, precision)
    code = train_arithmetic(precision).operand if (k - 1) * dil <= 32 else hip.F32      # beyond 32 rows of halo: the exact-f32 packing
    assert torch.equal(y, _explicit_conv(hip, rb, code, x, w, n_out, k, dil, pad, b, False))
    assert torch.equal(dx, _explicit_conv(hip, rb, code, gy, w, c_in, k, dil, (k - 1) * dil - pad, None, True))
    dw_ref, db_ref = hip.conv1d_wgrad(rb, x, gy, c_in, n_out, k, dil, pad, want_db=True, dtype=hip.F32)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)
    assert all(bool(torch.isfinite(t).all()) for t in (y, dx, dw, db))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_routed_weight_gradient_is_the_emulated_launch(cuda, lib, monkeypatch, shape):
    """The shape rule forced to True under fp32_bf16x3: the weight gradient is conv1d_wgrad(dtype=F32E) where the halo fits, the exact-f32 call where not."""
    from jatts_amd import autograd
    monkeypatch.setattr(autograd, "emul_wgrad_wins", lambda c_in, n_out, k, rows: True)
    c_in, n_out, k, dil = shape
    hip, rb, (w, x, b, gy), pad, (y, dx, dw, db) = _run(cuda, shape, "fp32_bf16x3")
    wcode = hip.F32E if (k - 1) * dil <= 32 else hip.F32
    dw_ref, db_ref = hip.conv1d_wgrad(rb, x, gy, c_in, n_out, k, dil, pad, want_db=True, dtype=wcode)
    assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)


def test_backward_after_the_context_launches_what_forward_decided(cuda, lib):
    """Forward inside arithmetic("fp32_bf16x3"), backward outside: dx is the emulated data-gradient launch, and differs from the exact-f32 one on this
    input (random normal data, the first seed tried), so the equality is not vacuous."""
    from jatts_amd import hip
    from jatts_amd.autograd import Conv1dFunction, arithmetic, current_arithmetic
    from jatts_amd.precision import TrainArithmetic
    c_in, n_out, k, dil = SHAPES[0]
    pad = (k - 1) // 2 * dil
    w, x, b, gy = _inputs(cuda, c_in, n_out, k)
    rb = hip.RaggedBatch(LENS, cuda)
    xd, wd = x.clone().requires_grad_(), w.clone().requires_grad_()
    with arithmetic("fp32_bf16x3"):
        y = Conv1dFunction.apply(xd, wd, b, rb, dil, pad)
    assert current_arithmetic() == TrainArithmetic(hip.F32, hip.F32)
    y.backward(gy)
    emul = _explicit_conv(hip, rb, hip.F32E, gy, w, c_in, k, dil, (k - 1) * dil - pad, None, True)
    exact = _explicit_conv(hip, rb, hip.F32, gy, w, c_in, k, dil, (k - 1) * dil - pad, None, True)
    assert torch.equal(xd.grad, emul)
    assert not torch.equal(xd.grad, exact)
