"""GPU: the free geometry of jatts_conv1d / jatts_conv1d_wgrad -- asymmetric and one-sided pad, even k_w, dil, rg.len_mul, summed inputs with
in_scale and the LeakyReLU prologue, x_col0 / out_col0 windows, f32 and f16 stores -- pinned at kernel level in every arithmetic.

The launches behind it: Matcha's folded stride-2 down-conv (k_w = 2, pad = 1) and training up-conv (k = 4, pad = 2; data gradient pad' = 1, weight
gradient on the VALU path), HiFi-GAN's polyphase upsampling convs (len_mul = rate, up to three inputs, in_scale = 1 / n, LeakyReLU prologue) and the
f16 row-major stores between the layers of every fp16 model.

Integer cases (tests/conv_geometry_cases.py; preconditions proven in tests/test_conv_geometry_cpu.py): the float64 result of the definition is the
expected output bit for bit in every arithmetic -- F32 (LDS-staged and register-streamed tiles), F16, F32S, F32E / F32E6 in both weight layouts and
every forced tile -- so one wrong row at a sequence edge, a halo read from the neighbouring utterance or an off-by-one under len_mul fails.  The
real-valued cases hold each arithmetic to the project's tolerances (tests/test_kernels_gpu.py, tests/test_emul_gpu.py): exact f32 relative L2
<= 2e-5, f16 <= 2e-3 on pre-rounded operands, split / emulated <= max(2e-5, 2 x the exact-f32 kernel's error), all against float64.
profiles/r12_notes.md: kernel -> case -> path, measured errors."""
import math

import pytest
import torch

import conv_geometry_cases as cg
from helpers import relerr

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-5, "fp16": 2e-3}          # the project's: tests/test_kernels_gpu.py
ARITHS = ["F32", "F16", "F32S", "F32E", "F32E6"]
NAN = float("nan")


# ------------------------------------------------------------------------------------------ one arithmetic = operand type, packed weight, launch variants
def _is_half(arith):
    return arith == "F16"


def _weights(hip, arith, w):
    """-> {w_layout: kwargs of hip.conv1d that carry the packed weight} for a device f32 weight (n_out, c_in, k)."""
    if arith == "F32":
        return {0: dict(w_packed=hip.pack_conv_weight(w, hip.F32), dtype=hip.F32)}
    if arith == "F16":
        return {0: dict(w_packed=hip.pack_conv_weight(w, hip.F16), dtype=hip.F16)}
    if arith == "F32S":
        wp, inv = hip.pack_conv_weight_split(w, 64)
        return {0: dict(w_packed=wp, w_inv=inv, dtype=hip.F32S)}
    code = getattr(hip, arith)
    return {0: dict(w_packed=hip.pack_conv_weight_bf16x3(w, 64), dtype=code, w_layout=0),
            1: dict(w_packed=hip.pack_conv_weight_bf16x3_k32(w, 64), dtype=code, w_layout=1)}


def _variants(arith, every_tile):
    """[(label, w_layout, kwargs)].  every_tile: each kernel / tile jatts_conv_desc.variant can force -- F32: 1 / 2 the LDS-staged 128 x 64 / 128 x 128 tiles,
    3 / 5 the register-streamed ones (they apply to one plain input, with or without the LeakyReLU prologue; any other launch falls back to the LDS-staged
    kernel and must still be right); emulated, w_layout 1: the tiles test_conv1d_emul16_tiles_agree forces (6, 3, 2, 1, 9)."""
    if arith == "F32":
        return [(f"v{v}", 0, dict(variant=v)) for v in ((0, 1, 2, 3, 5) if every_tile else (0,))]
    if arith == "F16":
        return [("y32", 0, dict(out_f32=True)), ("y16", 0, dict(out_f32=False))]
    if arith == "F32S":
        return [("", 0, {})]
    return [("l0", 0, {})] + [(f"l1v{v}", 1, dict(variant=v)) for v in ((0, 6, 3, 2, 1, 9) if every_tile else (0,))]


def _conv(hip, rb, xs, wkw, c_in, n_out, k, **kw):
    wkw = dict(wkw)
    return hip.conv1d(rb, xs, wkw.pop("w_packed"), c_in, n_out, k, **wkw, **kw)


# ------------------------------------------------------------------------------------------ the forward table
def _device_inputs(cfg, xs, dev, half):
    """-> (tensors, kwargs): the inputs on the device, as separate contiguous tensors or -- x_window -- as per-input x_col0 windows of ONE wider row
    whose other columns are NaN (a read outside a window poisons the output)."""
    dt = torch.float16 if half else torch.float32
    if not cfg.x_window:
        return [x.to(dt).to(dev).contiguous() for x in xs], {}
    ldx = 8 + cfg.n_in * cfg.c_in + 8
    wide = torch.full((xs[0].shape[0], ldx), NAN, dtype=dt)
    cols = [8 + i * cfg.c_in for i in range(cfg.n_in)]
    for c0, x in zip(cols, xs):
        wide[:, c0:c0 + cfg.c_in] = x.to(dt)
    wide = wide.to(dev)
    return [wide] * cfg.n_in, dict(ldx=ldx, x_col0=cols)


def _launch(hip, dev, geom, cfg, rb, xs, xkw, wkw, vkw, bias, half):
    """One jatts_conv1d launch of a table case -> the (rows, n_out) result.  With an out_window the output is a window of a wider NaN-prefilled
    buffer: every column outside it must still be NaN afterwards, every element inside finite."""
    k, dil, pad = geom
    kw = dict(dil=dil, pad=pad, bias=bias, act=hip.ACT_RELU if cfg.act == "relu" else hip.ACT_NONE, pre_lrelu=cfg.slope, in_scale=cfg.in_scale,
              len_mul=cfg.len_mul, **xkw, **vkw)
    if cfg.out_window is None:
        return _conv(hip, rb, xs, wkw, cfg.c_in, cfg.n_out, k, **kw)
    out_ld, col0 = cfg.out_window
    odt = torch.float16 if half and not vkw.get("out_f32") else torch.float32
    out = torch.full((rb.total * cfg.len_mul, out_ld), NAN, dtype=odt, device=dev)
    y = _conv(hip, rb, xs, wkw, cfg.c_in, cfg.n_out, k, out=out, out_ld=out_ld, out_col0=col0, **kw)
    assert y is out
    assert bool(torch.isnan(out[:, :col0]).all()) and bool(torch.isnan(out[:, col0 + cfg.n_out:]).all()), "stores outside the output window"
    win = out[:, col0:col0 + cfg.n_out]
    assert bool(torch.isfinite(win).all()), "unwritten elements inside the output window"
    return win.contiguous()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("gi", range(len(cg.GEOMS)), ids=cg.GEOM_IDS)
def test_conv1d_geometry_integer_exact(cuda, lib, gi, arith):
    """Every (k, dil, pad) of the table under every launch configuration (channel shape x len_mul x inputs / in_scale / prologue x windows), through
    every kernel and tile of the arithmetic: torch.equal with the integer reference."""
    from jatts_amd import hip
    for ci, cfg in enumerate(cg.CONFIGS):
        case = cg.forward_case(gi, ci)
        rb = hip.RaggedBatch(case.lens, cuda)
        xs, xkw = _device_inputs(cfg, case.xs, cuda, _is_half(arith))
        wk = _weights(hip, arith, case.w.to(cuda))
        bias = case.b.to(cuda)
        for label, layout, vkw in _variants(arith, every_tile=True):
            y = _launch(hip, cuda, case.geom, cfg, rb, xs, xkw, wk[layout], vkw, bias, _is_half(arith))
            assert y.dtype == (torch.float16 if label == "y16" else torch.float32)
            cg.check_exact(y, case.ref, f"{arith} {label} {cg.GEOM_IDS[gi]} {cfg.name}")


# ------------------------------------------------------------------------------------------ batch independence, real-valued
BATCH_GEOMS = [(4, 1, 2), (2, 1, 1), (3, 1, 0), (5, 2, 8), (7, 3, 5)]


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("geom", BATCH_GEOMS, ids=[f"k{k}d{d}p{p}" for k, d, p in BATCH_GEOMS])
def test_conv1d_sequence_alone_equals_inside_batch(cuda, lib, geom, arith):
    """Real-valued inputs (on integers the claim would follow from exactness): under an asymmetric pad and len_mul > 1 a sequence launched alone gives
    the bits it gives inside the batch -- the long one, one tile + 1 row, and the single-row one whose halo is all neighbours."""
    from jatts_amd import hip
    k, dil, pad = geom
    half = _is_half(arith)
    for cfg in (c for c in cg.CONFIGS if c.len_mul > 1):
        g = cg._gen("alone", geom, cfg.name)
        lens = cg.lens_of(geom, cfg)
        rows = sum(lens) * cfg.len_mul
        xs = [torch.randn(rows, cfg.c_in, generator=g) for _ in range(cfg.n_in)]
        w = torch.randn(cfg.n_out, cfg.c_in, k, generator=g) / math.sqrt(cfg.c_in * k)
        bias = torch.randn(cfg.n_out, generator=g).to(cuda)
        wk = _weights(hip, arith, w.to(cuda))
        for label, layout, vkw in _variants(arith, every_tile=False):
            dxs, xkw = _device_inputs(cfg, xs, cuda, half)
            y = _launch(hip, cuda, geom, cfg, hip.RaggedBatch(lens, cuda), dxs, xkw, wk[layout], vkw, bias, half)
            cu = [0]
            for v in lens:
                cu.append(cu[-1] + v * cfg.len_mul)
            for b in (0, 2, 1):
                one, okw = _device_inputs(cfg, [x[cu[b]:cu[b + 1]] for x in xs], cuda, half)
                ya = _launch(hip, cuda, geom, cfg, hip.RaggedBatch([lens[b]], cuda), one, okw, wk[layout], vkw, bias, half)
                assert torch.equal(ya, y[cu[b]:cu[b + 1]]), f"{arith} {label} {cfg.name}: sequence {b} (length {lens[b]} x {cfg.len_mul}) differs alone / in the batch"


# ------------------------------------------------------------------------------------------ the product's forms
@pytest.mark.parametrize("arith", ARITHS)
def test_folded_stride2_conv_equals_the_strided_conv(cuda, lib, arith):
    """Matcha's down-conv: Conv1d(C, C, 3, stride 2, padding 1) run as k_w = 2, pad = 1 over pair rows -- against F.conv1d(stride=2, padding=1) on the
    unfolded signal, integer-exact."""
    from jatts_amd import hip
    half = _is_half(arith)
    for C0 in cg.STRIDE2_CHANNELS:
        case = cg.stride2_case(C0)
        rb2 = hip.RaggedBatch(cg.STRIDE2_PAIR_LENS, cuda)
        x = case.x.to(torch.float16 if half else torch.float32).to(cuda).view(-1, 2 * C0)
        wk = _weights(hip, arith, cg.fold_stride2(case.wd).to(cuda))
        for label, layout, vkw in _variants(arith, every_tile=True):
            y = _conv(hip, rb2, x, wk[layout], 2 * C0, C0, 2, pad=1, bias=case.b.to(cuda), **vkw)
            cg.check_exact(y, case.ref, f"{arith} {label} folded stride-2 conv, C = {C0}")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("chain", range(len(cg.POLY_CHAINS)), ids=cg.POLY_CHAIN_IDS)
def test_polyphase_chain_equals_conv_transpose(cuda, lib, chain, arith):
    """Two chained polyphase stages as HiFi-GAN launches them (hip.convtranspose_as_conv, bias repeated per phase, the second stage at len_mul = s1 on the
    [s1][c] row view of the first) against conv_transpose1d stage after stage, integer-exact; the f16 arithmetic hands f16 rows from stage to stage."""
    from jatts_amd import hip
    half = _is_half(arith)
    case = cg.poly_case(chain)
    rb = hip.RaggedBatch(cg.POLY_LENS, cuda)
    for label, layout, vkw in _variants(arith, every_tile=False):
        if label == "y32":
            continue       # (between layers the f16 models store f16)
        h, rate = case.x.to(torch.float16 if half else torch.float32).to(cuda), 1
        for (w, b, s), want in zip(case.stages, (case.mid, case.ref)):
            wc, pad = hip.convtranspose_as_conv(w, s, cg.poly_padding(s))
            wk = _weights(hip, arith, wc.to(cuda))
            y = _conv(hip, rb, h, wk[layout], w.shape[0], s * w.shape[1], wc.shape[-1], pad=pad, bias=b.repeat(s).to(cuda), len_mul=rate, **vkw)
            rate *= s
            h = y.view(rb.total * rate, w.shape[1])
            cg.check_exact(h, want, f"{arith} {label} polyphase stage s = {s}, K = {w.shape[2]}, len_mul = {rate // s}")


REAL_GEOM, REAL_CFG = (4, 1, 2), cg.Config("real", 192, 160, 1, 1.0, None, "relu", 2, True, (184, 8), 64, 200)


@pytest.fixture(scope="module")
def real_case():
    """One random-real launch (asymmetric pad, len_mul 2, windows on both sides) and its float64 reference; f16 operands pre-rounded."""
    k, dil, pad = REAL_GEOM
    g = cg._gen("real")
    lens = cg.lens_of(REAL_GEOM, REAL_CFG)
    row_lens = [v * REAL_CFG.len_mul for v in lens]
    x = torch.randn(sum(row_lens), REAL_CFG.c_in, generator=g)
    w = torch.randn(REAL_CFG.n_out, REAL_CFG.c_in, k, generator=g) / math.sqrt(REAL_CFG.c_in * k)
    b = torch.randn(REAL_CFG.n_out, generator=g)
    out = {}
    for half in (False, True):
        xr, wr = (x.half().float(), w.half().float()) if half else (x, w)
        out[half] = (xr, wr, cg.reference_conv(xr, wr, b, row_lens, k, dil, pad, "relu"))
    return lens, b, out


@pytest.mark.parametrize("arith", ARITHS)
def test_conv1d_geometry_real_valued(cuda, lib, real_case, arith):
    from jatts_amd import hip
    lens, b, per = real_case
    half = _is_half(arith)
    x, w, ref = per[half]
    rb = hip.RaggedBatch(lens, cuda)

    def run(a, layout, vkw):
        xs, xkw = _device_inputs(REAL_CFG, [x], cuda, _is_half(a))
        return _launch(hip, cuda, REAL_GEOM, REAL_CFG, rb, xs, xkw, _weights(hip, a, w.to(cuda))[layout], vkw, b.to(cuda), _is_half(a))
    e32 = relerr(run("F32", 0, {}), per[False][2]) if not half else None
    for label, layout, vkw in _variants(arith, every_tile=False):
        e = relerr(run(arith, layout, vkw), ref)
        print(f"conv geometry real-valued {arith} {label}: rel L2 {e:.3e}" + ("" if e32 is None else f" (exact f32 {e32:.3e})"))
        if arith == "F32":
            assert e <= TOL["fp32"]
        elif arith == "F16":
            assert e <= TOL["fp16"]                   # f32 and f16 stores alike
        else:
            assert e <= max(TOL["fp32"], 2.0 * e32), f"{arith} {label}: rel err {e:.3e} (exact f32 {e32:.3e})"


# ------------------------------------------------------------------------------------------ backward
def _modes():
    import contextlib
    import functools
    from jatts_amd.autograd import arithmetic
    return {"exact": contextlib.nullcontext, "split": functools.partial(arithmetic, "fp32_split"), "emul": functools.partial(arithmetic, "fp32_bf16x3")}


@pytest.mark.parametrize("mode", ["exact", "split", "emul"])
@pytest.mark.parametrize("geom", cg.BACKWARD_GEOMS, ids=[f"k{k}d{d}p{p}" for k, d, p in cg.BACKWARD_GEOMS])
def test_conv1d_function_backward_geometry(cuda, lib, geom, mode):
    """Conv1dFunction (forward, data gradient = the same kernel at pad' = (k - 1) dil - pad, weight / bias gradient) against float64 autograd through the
    explicitly padded conv, on integers: y, dx, dW, db are exact in all three modes (operands of at most 4 bits, sums below 2**24).  The two
    geometries with a halo beyond 32 rows take the exact-f32 fallback of the split and emulated modes."""
    from jatts_amd import hip
    from jatts_amd.autograd import Conv1dFunction
    k, dil, pad = geom
    lens = cg.wgrad_lens(geom, 1)
    rb = hip.RaggedBatch(lens, cuda)
    for c_in, n_out in cg.WGRAD_SHAPES:
        g = cg._gen("bwd", geom, c_in)
        x = torch.randint(-8, 9, (sum(lens), c_in), generator=g).float()
        w, b = cg.int_weight(n_out, c_in, k, g)
        gy = torch.randint(-4, 5, (sum(lens), n_out), generator=g).float()
        xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
        yr = cg.reference_conv(xr, wr, br, lens, k, dil, pad)
        yr.backward(gy.double())
        assert max(float(t.abs().max()) for t in (yr.detach(), xr.grad, wr.grad, br.grad)) < cg.F24
        xd, wd, bd = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
        with _modes()[mode]():
            y = Conv1dFunction.apply(xd, wd, bd, rb, dil, pad)
            y.backward(gy.to(cuda))
        for name, got, want in (("y", y, yr), ("dx", xd.grad, xr.grad), ("dW", wd.grad, wr.grad), ("db", bd.grad, br.grad)):
            cg.check_exact(got.view(got.shape[0], -1), want.detach().view(want.shape[0], -1), f"{mode} {name} k{k}d{dil}p{pad} {c_in}->{n_out}")


@pytest.mark.parametrize("dtype", ["F32", "F32E"])
@pytest.mark.parametrize("gi", range(len(cg.WGRAD_GEOMS)), ids=[f"k{k}d{d}p{p}" for k, d, p in cg.WGRAD_GEOMS])
def test_conv1d_wgrad_geometry(cuda, lib, gi, dtype):
    """hip.conv1d_wgrad itself: k 1 / 3 / 5 on the MFMA path (F32E: the emulated kernel), k 2 / 4 / 7 on the VALU path (F32E: through the exact-f32 entry),
    len_mul 1 and 4, asymmetric pad, with and without the bias gradient: integer-exact, and two launches give the same bits."""
    from jatts_amd import hip
    code = getattr(hip, dtype)
    k, dil, pad = cg.WGRAD_GEOMS[gi]
    for si, (c_in, n_out) in enumerate(cg.WGRAD_SHAPES):
        for len_mul in (1, 4):
            case = cg.wgrad_case(gi, si, len_mul)
            rb = hip.RaggedBatch(case.lens, cuda)
            x, dy = case.x.to(cuda), case.dy.to(cuda)
            what = f"{dtype} k{k}d{dil}p{pad} {c_in}->{n_out} len_mul {len_mul}"
            dw, db = hip.conv1d_wgrad(rb, x, dy, c_in, n_out, k, dil, pad, len_mul=len_mul, want_db=True, dtype=code)
            cg.check_exact(dw.view(n_out, -1), case.dw.view(n_out, -1), what + " dW")
            cg.check_exact(db.view(-1, 1), case.db.view(-1, 1), what + " db")
            dw2, db2 = hip.conv1d_wgrad(rb, x, dy, c_in, n_out, k, dil, pad, len_mul=len_mul, want_db=True, dtype=code)
            assert torch.equal(dw2, dw) and torch.equal(db2, db), what + ": two launches differ"
            dw3 = hip.conv1d_wgrad(rb, x, dy, c_in, n_out, k, dil, pad, len_mul=len_mul, want_db=False, dtype=code)
            assert torch.equal(dw3, dw), what + ": dW depends on want_db"


@pytest.mark.parametrize("dtype", ["F32", "F32E"])
@pytest.mark.parametrize("k,dil", [(3, 1), (5, 2), (4, 1), (7, 3)])
def test_conv1d_wgrad_taps_that_see_only_padding_are_zero(cuda, lib, k, dil, dtype):
    """Single-row sequences: with pad = 0 only tap 0 ever meets a row of its own sequence, with pad = (k - 1) dil only the last tap -- every other tap of
    dW is exactly zero (not the neighbouring utterance's row), and the live tap is the per-row outer product summed."""
    from jatts_amd import hip
    code = getattr(hip, dtype)
    g = cg._gen("zerotaps", k, dil)
    lens = [1] * 9
    rb = hip.RaggedBatch(lens, cuda)
    for c_in, n_out in cg.WGRAD_SHAPES:
        x = torch.randint(-8, 9, (len(lens), c_in), generator=g).float()
        dy = torch.randint(-4, 5, (len(lens), n_out), generator=g).float()
        live = dy.double().t() @ x.double()
        for pad, tap in ((0, 0), ((k - 1) * dil, k - 1)):
            dw = hip.conv1d_wgrad(rb, x.to(cuda), dy.to(cuda), c_in, n_out, k, dil, pad, dtype=code).cpu()
            dead = [t for t in range(k) if t != tap]
            assert not bool(dw[:, :, dead].any()), f"{dtype} k{k} pad {pad}: taps that see only padding are not zero"
            cg.check_exact(dw[:, :, tap], live, f"{dtype} k{k} pad {pad} tap {tap}")
            want, _ = cg.reference_wgrad(x, dy, lens, k, dil, pad)
            cg.check_exact(dw.view(n_out, -1), want.view(n_out, -1), f"{dtype} k{k} pad {pad}")


# ------------------------------------------------------------------------------------------ sensitivity on the device
@pytest.mark.parametrize("arith", ARITHS)
def test_wrong_geometry_is_rejected_on_the_device(cuda, lib, arith):
    """The kernels themselves launched with a geometry that is wrong by one row -- an (in-range) pad one off, and the batch merged into ONE sequence so
    that every halo reads its neighbours -- give results check_exact rejects, in every arithmetic and layout; the right launch next to each is accepted."""
    from jatts_amd import hip
    half = _is_half(arith)
    for gi in (0, 2, 4, 7, 9):
        for ci in (0, 2, 3):
            case = cg.forward_case(gi, ci)
            cfg = case.cfg
            k, dil, pad = case.geom
            xs, xkw = _device_inputs(cfg, case.xs, cuda, half)
            wk = _weights(hip, arith, case.w.to(cuda))
            bias = case.b.to(cuda)
            wrong_pad = pad + 1 if pad < (k - 1) * dil else pad - 1
            for label, layout, vkw in _variants(arith, every_tile=False):
                what = f"{arith} {label} {cg.GEOM_IDS[gi]} {cfg.name}"
                y = _launch(hip, cuda, case.geom, cfg, hip.RaggedBatch(case.lens, cuda), xs, xkw, wk[layout], vkw, bias, half)
                cg.check_exact(y, case.ref, what)
                for name, geom, lens in (("pad off by one", (k, dil, wrong_pad), case.lens), ("merged batch", case.geom, [sum(case.lens)])):
                    y = _launch(hip, cuda, geom, cfg, hip.RaggedBatch(lens, cuda), xs, xkw, wk[layout], vkw, bias, half)
                    with pytest.raises(AssertionError, match="differ from the integer reference"):
                        cg.check_exact(y, case.ref, f"{what} {name}")
