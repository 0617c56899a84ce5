"""GPU parity of the SINGLE-CONV HiFi-GAN dilation unit (jatts_hifigan_resunit with w2 == NULL; csrc/resunit1_*):

    y = out_scale_mix( x + conv_k,d( lrelu(x) ) + b1 )

in its four arithmetics -- exact f32 (JATTS_F32), seven / six bf16x3 products (JATTS_F32E / JATTS_F32E6, w_layout 1) and f16 -- through
hip.hifigan_resunit(..., w2=None, b2=None).  Reference: per utterance in float64; for f16, x, w and lrelu(x) rounded to f16 beforehand (as
test_kernels_gpu._ref_unit(round16=True)).  y is prefilled with NaN.

Tolerances are the project's own (tests/test_kernels_gpu.py TOL, tests/test_emul_gpu.py): f32 relative L2 <= 2e-5, f16 <= 2e-3; seven products: relative L2
<= max(2e-5, 2 x the exact-f32 single-conv kernel's), maximum error <= 2 x its; six products: relative L2 <= 2e-5 and maximum error <= 2 x the exact
kernel's (single-non-zero rows: relative L2 <= 3 x).  Single-non-zero weights: every element within PER_PRODUCT 2^-24 |w u| + 2^-24 |y|  (u = lrelu(x) as
the f32 operand the kernel splits; the second term is the one rounded residual add).
"""
import functools
import math
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL = {"f32": 2e-5, "f16": 2e-3}
PER_PRODUCT = {"7": 2.01, "6": 4.01}      # tests/test_emul_gpu.py
ARITHS = ["f32", "e7", "e6", "f16"]
SLOPE = 0.1

# (C, k, d, lens): more than two windows of every tile, utterances of 1 and 2 rows and shorter than the halo, the halo past 32 rows a side (k = 7, d = 12),
# the channel-half tile (256, 11, 5)
CASES = [
    (32, 3, 1, [700, 3, 250]), (32, 7, 12, [600, 31, 1]), (64, 5, 6, [513, 2]), (64, 7, 12, [300, 35]), (64, 11, 5, [260, 9]),
    (128, 3, 2, [300, 40]), (128, 7, 12, [200, 71, 1]), (128, 11, 5, [129]), (256, 7, 3, [150, 64]), (256, 11, 5, [70, 49]),
    # the instantiations the list above does not reach: f32 C = 128 k > 7 on the 128-column window, f16 C = 32 k > 7, f16 C = 64 k = 3
    (128, 11, 1, [300, 40]), (32, 11, 3, [1100, 5]), (64, 3, 5, [600, 1]),
    (512, 3, 3, [45]),          # f16 only
]
# window width (columns per workgroup) of the kernel each (arithmetic class, C, k, d) launches: csrc/resunit1_f32.hip, resunit1_f16.hip, resunit1_emul.hip
WINDOW = {
    "f32": {(32, 3, 1): 512, (32, 7, 12): 512, (64, 5, 6): 256, (64, 7, 12): 256, (64, 11, 5): 256, (128, 3, 2): 128, (128, 7, 12): 128, (128, 11, 5): 256,
            (256, 7, 3): 128, (256, 11, 5): 96, (128, 11, 1): 128, (32, 11, 3): 512, (64, 3, 5): 256},
    "f16": {(32, 3, 1): 256, (32, 7, 12): 256, (64, 5, 6): 512, (64, 7, 12): 512, (64, 11, 5): 512, (128, 3, 2): 256, (128, 7, 12): 192, (128, 11, 5): 192,
            (256, 7, 3): 128, (256, 11, 5): 128, (128, 11, 1): 256, (32, 11, 3): 512, (64, 3, 5): 256, (512, 3, 3): 32},
    "emul": {(32, 3, 1): 256, (32, 7, 12): 256, (64, 5, 6): 128, (64, 7, 12): 128, (64, 11, 5): 256, (128, 3, 2): 128, (128, 7, 12): 128, (128, 11, 5): 128,
             (256, 7, 3): 64, (256, 11, 5): 64, (128, 11, 1): 128, (32, 11, 3): 256, (64, 3, 5): 128},
}


def _cls(arith):
    return "emul" if arith in ("e7", "e6") else arith


def _code(hip, arith):
    return {"f32": hip.F32, "e7": hip.F32E, "e6": hip.F32E6, "f16": hip.F16}[arith]


def _pack(hip, w, arith):
    if arith in ("e7", "e6"):
        return hip.pack_unit_weight_bf16x3_k32(w)
    return hip.pack_conv_weight(w, _code(hip, arith), 32)


def _lrelu_operand(x, slope, round16):
    """lrelu(x) as the operand the kernel contracts: max(x, x * slope) with the product rounded once in the activation's format."""
    if round16:
        h = x.half()
        return torch.maximum(h, (h.float() * slope).half()).double()
    return torch.maximum(x, x * torch.tensor(slope, dtype=torch.float32)).double()


def _ref(x, w, b, lens, k, d, slope, round16, operand=False):
    """float64 per utterance: x + conv_k,d(lrelu(x)) + b.  operand=True: lrelu taken as the rounded operand (the single-non-zero element bound)."""
    outs, o = [], 0
    for L in lens:
        xs = x[o:o + L].t().unsqueeze(0)
        if operand:
            a = _lrelu_operand(xs, slope, round16)
        else:
            a = F.leaky_relu(xs.double(), slope)
            if round16:
                a = a.half().double()
        y = F.conv1d(a, w.double(), None if b is None else b.double(), padding=(k - 1) // 2 * d, dilation=d) + xs.double()
        outs.append(y[0].t())
        o += L
    return torch.cat(outs)


@functools.lru_cache(maxsize=None)
def _inputs(C, k, d, lens, round16, single=False):
    """x, w, b, float64 reference (computed once per case, shared and left unchanged)."""
    g = torch.Generator().manual_seed(C * 100 + k * 10 + d + (7 if single else 0))
    R = sum(lens)
    x = torch.randn(R, C, generator=g)
    w = torch.randn(C, C, k, generator=g) / math.sqrt(C * k) * torch.pow(10.0, torch.rand(C, 1, 1, generator=g) * 2 - 1)   # per-channel spread
    b = torch.randn(C, generator=g) * 0.1
    if single:
        from tools.emul_sweep import single_nonzero_
        single_nonzero_(w, g).mul_(math.sqrt(C * k))
        b = None
    if round16:
        x, w = x.half().float(), w.half().float()
    return x, w, b, _ref(x, w, b, list(lens), k, d, SLOPE, round16)


def _run(hip, cuda, arith, x, w, b, lens, C, k, d, slope=SLOPE, add=None, out_scale=1.0, len_mul=1):
    code = _code(hip, arith)
    tdt = hip.torch_dtype(code)
    xd = x.to(cuda).to(tdt)
    y = torch.full_like(xd, float("nan"))
    bd = (torch.zeros(C) if b is None else b).to(cuda)
    hip.hifigan_resunit(hip.RaggedBatch(lens, cuda), len_mul, xd, y, _pack(hip, w.to(cuda), arith), bd, None, None, C, k, d, slope, code,
                        add=None if add is None else [a.to(cuda).to(tdt) for a in add], out_scale=out_scale, w_layout=1 if _cls(arith) == "emul" else 0)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), "unwritten / non-finite outputs"
    return y


def _maxerr(y, ref):
    return float((y.double().cpu() - ref).abs().max())


def _check(hip, cuda, arith, y, ref, what, y32=None):
    e = relerr(y.float(), ref)
    print(f"{what} {arith}: rel L2 {e:.3e} max {_maxerr(y, ref):.3e}" + (f" (exact f32: {relerr(y32, ref):.3e} / {_maxerr(y32, ref):.3e})" if y32 is not None else ""))
    if arith in ("f32", "f16"):
        assert e <= TOL[arith], f"{what} {arith}: rel err {e:.3e}"
        return
    e32, m, m32 = relerr(y32, ref), _maxerr(y, ref), _maxerr(y32, ref)
    if arith == "e7":
        assert e <= max(TOL["f32"], 2.0 * e32), f"{what} e7: rel L2 {e:.3e} vs exact f32 {e32:.3e}"
    else:
        assert e <= TOL["f32"], f"{what} e6: rel L2 {e:.3e} (exact f32 {e32:.3e})"
    assert m <= 2.0 * m32 + 1e-30, f"{what} {arith}: max err {m:.3e} vs exact f32 {m32:.3e}"


# 512 channels: f16 only (the other arithmetics have no 512-channel tile; test_resunit1_refusals)
CASE_ARITHS = [pytest.param(C, k, d, lens, a, id=f"C{C}-k{k}-d{d}-{a}") for C, k, d, lens in CASES for a in ARITHS if C <= 256 or a == "f16"]


@pytest.mark.parametrize("lens_kind", ["case", "window"])
@pytest.mark.parametrize("C,k,d,lens,arith", CASE_ARITHS)
def test_resunit1_matches_float64(cuda, lib, C, k, d, lens, arith, lens_kind):
    """Every case in every arithmetic, at the case's lengths and at [T - 1, T, T + 1] of the launched kernel's window width T; an utterance alone is
    bit-identical to the same utterance inside the batch."""
    from jatts_amd import hip
    if lens_kind == "window":
        T = WINDOW[_cls(arith)][(C, k, d)]
        lens = [T - 1, T, T + 1]
    x, w, b, ref = _inputs(C, k, d, tuple(lens), arith == "f16")
    y = _run(hip, cuda, arith, x, w, b, lens, C, k, d)
    y32 = _run(hip, cuda, "f32", x, w, b, lens, C, k, d) if _cls(arith) == "emul" else None
    _check(hip, cuda, arith, y, ref, f"resunit1 C={C} k={k} d={d} {lens}", y32)
    if len(lens) > 1:
        i = 1 if lens_kind == "case" else 2           # (case lists: the short second utterance; windows: T + 1)
        o = sum(lens[:i])
        y0 = _run(hip, cuda, arith, x[o:o + lens[i]], w, b, [lens[i]], C, k, d)
        assert torch.equal(y0, y[o:o + lens[i]])
        y0 = _run(hip, cuda, arith, x[:lens[0]], w, b, [lens[0]], C, k, d)
        assert torch.equal(y0, y[:lens[0]])


@pytest.mark.parametrize("np_", ["7", "6"])
@pytest.mark.parametrize("C,k,d,lens", [c for c in CASES if c[0] <= 256], ids=[f"C{c}-k{k}-d{d}" for c, k, d, _ in CASES if c <= 256])
def test_resunit1_single_nonzero_weights(cuda, lib, C, k, d, lens, np_):
    """One non-zero weight per output channel, no bias: every contraction has one term, so every element lies within
    PER_PRODUCT 2^-24 |w u| (the dropped partial products and the accumulator's roundings) + 2^-24 |y| (the one rounded residual add)."""
    from jatts_amd import hip
    arith = "e" + np_
    x, w, _, ref = _inputs(C, k, d, tuple(lens), False, True)
    y = _run(hip, cuda, arith, x, w, None, lens, C, k, d)
    y32 = _run(hip, cuda, "f32", x, w, None, lens, C, k, d)
    e, e32 = relerr(y, ref), relerr(y32, ref)
    print(f"single C={C} k={k} d={d} {arith}: rel L2 {e:.3e} (exact f32 {e32:.3e})")
    assert e <= TOL["f32"]
    assert e <= (2.0 if np_ == "7" else 3.0) * e32 + 1e-30, f"rel L2 {e:.3e} vs exact f32 {e32:.3e}"
    refo = _ref(x, w, None, lens, k, d, SLOPE, False, operand=True)
    wu = (refo - x.double()).abs()                     # the one product of each element (0 where the tap falls outside the utterance)
    err = (y.double().cpu() - refo).abs()
    bound = PER_PRODUCT[np_] * 2.0 ** -24 * wu + 2.0 ** -24 * refo.abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"single C={C} k={k} d={d} {arith}: worst element at {worst:.3f} of its bound")
    assert (err <= bound).all(), f"element at {worst:.3f} of its bound"


@pytest.mark.parametrize("arith", ARITHS)
def test_resunit1_len_mul(cuda, lib, arith):
    """len_mul = 8 on base lengths [40, 1, 17] == the same rows passed as plain lengths."""
    from jatts_amd import hip
    C, k, d, base = 64, 7, 12, [40, 1, 17]
    lens = [8 * n for n in base]
    x, w, b, ref = _inputs(C, k, d, tuple(lens), arith == "f16")
    y = _run(hip, cuda, arith, x, w, b, lens, C, k, d)
    y8 = _run(hip, cuda, arith, x, w, b, base, C, k, d, len_mul=8)
    assert torch.equal(y, y8)
    y32 = _run(hip, cuda, "f32", x, w, b, lens, C, k, d) if _cls(arith) == "emul" else None
    _check(hip, cuda, arith, y8, ref, "len_mul", y32)


@pytest.mark.parametrize("n_add,scale", [(1, 0.5), (2, 1.0 / 3.0)])
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("C,k,d,lens", [(32, 7, 12, [600, 31, 1]), (128, 3, 2, [300, 40]), (256, 11, 5, [70, 49])])
def test_resunit1_mrf_mix(cuda, lib, C, k, d, lens, arith, n_add, scale):
    """The fused MRF mean y = out_scale (unit(x) + add0 [+ add1]) against float64, at the unit's own tolerances (residual-register, store-pass and
    channel-half tiles)."""
    from jatts_amd import hip
    x, w, b, ref = _inputs(C, k, d, tuple(lens), arith == "f16")
    g = torch.Generator().manual_seed(n_add)
    add = [torch.randn(sum(lens), C, generator=g) for _ in range(n_add)]
    if arith == "f16":
        add = [a.half().float() for a in add]
    refm = (ref + sum(a.double() for a in add)) * scale
    y = _run(hip, cuda, arith, x, w, b, lens, C, k, d, add=add, out_scale=scale)
    y32 = _run(hip, cuda, "f32", x, w, b, lens, C, k, d, add=add, out_scale=scale) if _cls(arith) == "emul" else None
    _check(hip, cuda, arith, y, refm, f"mrf C={C} n_add={n_add}", y32)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("C,k,d,lens", [(32, 7, 12, [600, 31, 1]), (64, 5, 6, [513, 2]), (128, 11, 5, [300]), (256, 11, 5, [70, 49])])
def test_resunit1_integers_exact(cuda, lib, C, k, d, lens, arith):
    """Integer data on which every arithmetic is exact: slope 0.25, negative x in multiples of 4 with |lrelu(x)| <= 8, integer |w| <= 4 (at most 24
    non-zero per output channel), integer bias.  The bounds are proven from the tensors: every partial sum, the conv + bias and y stay below 2^24
    (f32 accumulators exact) and below 2048 (f16 stores exact; bf16 terms: |u| <= 8 and |w| <= 4 are one-term values).  torch.equal, also with the
    MRF mix at out_scale = 1."""
    from jatts_amd import hip
    g = torch.Generator().manual_seed(C + k + d)
    R = sum(lens)
    pos = torch.randint(0, 9, (R, C), generator=g).float()
    neg = -4.0 * torch.randint(1, 9, (R, C), generator=g).float()
    x = torch.where(torch.rand(R, C, generator=g) < 0.5, pos, neg)
    w = torch.zeros(C, C * k)
    for n in range(C):
        idx = torch.randperm(C * k, generator=g)[:24]
        w[n, idx] = torch.randint(-4, 5, (24,), generator=g).float()
    w = w.view(C, C, k)
    b = torch.randint(-8, 9, (C,), generator=g).float()
    add = [torch.randint(-16, 17, (R, C), generator=g).float() for _ in range(2)]
    u = F.leaky_relu(x, 0.25)
    assert float(u.abs().max()) <= 8 and torch.equal(u, u.round()) and float(w.abs().max()) <= 4
    bound = float(u.abs().max() * w.abs().sum((1, 2)).max() + b.abs().max() + x.abs().max())
    bound_mix = bound + sum(float(a.abs().max()) for a in add)
    assert bound_mix < 2 ** 24
    assert bound_mix < 2048            # f16: every intermediate and |y| are exact f16 integers
    ref = _ref(x, w, b, lens, k, d, 0.25, False)
    assert float(ref.abs().max()) <= bound
    y = _run(hip, cuda, arith, x, w, b, lens, C, k, d, slope=0.25)
    assert torch.equal(y.double().cpu(), ref)
    for n_add in (1, 2):
        ym = _run(hip, cuda, arith, x, w, b, lens, C, k, d, slope=0.25, add=add[:n_add], out_scale=1.0)
        assert torch.equal(ym.double().cpu(), ref + sum(a.double() for a in add[:n_add]))


def test_resunit1_refusals(cuda, lib):
    """Refused by the argument / shape checks that run before any launch (y, prefilled with NaN, stays untouched): b2 without w2 is an argument error;
    the split arithmetic and the w_layout = 0 emulated form have no single-conv kernel; the form reported is windowed."""
    from jatts_amd import _abi, hip
    ERR_ARG, ERR_UNSUPPORTED = -1, -3         # include/jatts_hip.h
    C, k, d = 64, 3, 1
    rb = hip.RaggedBatch([8], cuda)
    x = torch.zeros(8, C, device=cuda)
    y = torch.full((8, C), float("nan"), device=cuda)
    w = torch.randn(C, C, k, device=cuda)
    b = torch.zeros(C, device=cuda)

    def code_of(fn):
        try:
            fn()
        except _abi.JattsHipError as e:
            return int(re.search(r"rc=(-?\d+)", str(e)).group(1))
        return 0

    e = code_of(lambda: hip.hifigan_resunit(rb, 1, x, y, hip.pack_conv_weight(w, hip.F32, 32), b, None, b, C, k, d, 0.1, hip.F32))
    assert e == ERR_ARG, e
    ws, inv = hip.pack_conv_weight_split(w, 32)
    e = code_of(lambda: hip.hifigan_resunit(rb, 1, x, y, ws, b, None, None, C, k, d, 0.1, hip.F32S, ws=(inv,)))
    assert e == ERR_UNSUPPORTED, e
    e = code_of(lambda: hip.hifigan_resunit(rb, 1, x, y, hip.pack_conv_weight_bf16x3(w, 32), b, None, None, C, k, d, 0.1, hip.F32E, w_layout=0))
    assert e == ERR_UNSUPPORTED, e
    torch.cuda.synchronize()
    assert torch.isnan(y).all()               # nothing launched
    # the supported form of the same batch runs, and the form is windowed whatever is asked
    hip.hifigan_resunit(rb, 1, x, y, hip.pack_unit_weight_bf16x3_k32(w), b, None, None, C, k, d, 0.1, hip.F32E, w_layout=1)
    assert not y.any()
    rb1 = hip.RaggedBatch([4000], cuda)
    x1 = torch.zeros(4000, C, device=cuda)
    for variant in (0, 1, 2):
        assert hip.resunit_variant(rb1, 1, x1, torch.empty_like(x1), hip.pack_unit_weight_bf16x3_k32(w), b, None, None, C, k, d, 0.1, hip.F32E,
                                   w_layout=1, variant=variant) == 1
    # a window that cannot fit 160 KiB is refused by the shape check, before the launch: C = 256, (k - 1) d = 72 in exact f32
    C2 = 256
    x2 = torch.zeros(64, C2, device=cuda)
    e = code_of(lambda: hip.hifigan_resunit(hip.RaggedBatch([64], cuda), 1, x2, torch.empty_like(x2), torch.zeros(C2 * C2 * 7, device=cuda),
                                            torch.zeros(C2, device=cuda), None, None, C2, 7, 12, 0.1, hip.F32))
    assert e == ERR_UNSUPPORTED, e
    # 512 channels: f16 only
    x3 = torch.zeros(8, 512, device=cuda)
    e = code_of(lambda: hip.hifigan_resunit(hip.RaggedBatch([8], cuda), 1, x3, torch.empty_like(x3), torch.zeros(512 * 512 * 3, device=cuda),
                                            torch.zeros(512, device=cuda), None, None, 512, 3, 1, 0.1, hip.F32))
    assert e == ERR_UNSUPPORTED, e
