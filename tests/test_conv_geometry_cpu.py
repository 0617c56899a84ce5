"""No GPU: the preconditions and references of tests/test_conv_geometry_gpu.py (tests/conv_geometry_cases.py).

 * Every case of the tables satisfies what makes its float64 reference THE answer in every arithmetic: integer operands of at most 11 bits,
   sum |w| |u| + |b| < 2**24 (no partial sum can round, in any order), |y| < 2048 (an f16 store does not round either).
 * The references agree with each other where two formulations of one operation exist: the folded k_w = 2, pad = 1 conv over pair rows is the
   stride-2 conv; the polyphase conv is conv_transpose1d, chained over two stages with the second at len_mul = s1.
 * The comparison the GPU tests use rejects a geometry that is wrong by one row."""
import ctypes as C

import pytest
import torch

import conv_geometry_cases as cg


def _is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("ci", range(len(cg.CONFIGS)), ids=cg.CONFIG_IDS)
@pytest.mark.parametrize("gi", range(len(cg.GEOMS)), ids=cg.GEOM_IDS)
def test_forward_cases_are_exact_in_every_arithmetic(gi, ci):
    case = cg.forward_case(gi, ci)
    k, dil, pad = case.geom
    cfg = case.cfg
    assert 0 <= pad <= (k - 1) * dil
    # operands: integers of at most 11 bits (f16 holds them), the staged operand |u| <= 8, |w| <= 4, integer bias
    for x in case.xs:
        assert _is_int(x) and float(x.abs().max()) < cg.F16_EXACT
    assert _is_int(case.u) and float(case.u.abs().max()) <= 8
    assert _is_int(case.w) and float(case.w.abs().max()) <= 4 and _is_int(case.b)
    # the staged operand is what the kernels compute from the inputs: in_scale * sum, then max(v, slope v); every step exact in f32
    v = sum(case.xs) * cfg.in_scale
    staged = torch.maximum(v, v * cfg.slope) if cfg.slope is not None else v
    assert torch.equal(staged.double(), case.u)
    assert float((sum(x.abs() for x in case.xs)).max()) < cg.F16_EXACT          # the f32 sum of the inputs, before the scale
    # no partial sum can reach 2**24; the result fits f16
    assert cg.abs_bound(case) < cg.F24
    assert _is_int(case.ref) and float(case.ref.abs().max()) < cg.F16_EXACT
    # the batch holds what the issue asks for: 1, 2, a length below the halo, a tile width +- 1, a few hundred rows; and stays small
    t = cfg.tile
    assert {1, 2, t - 1, t, t + 1} <= set(case.lens) and max(case.lens) >= 100 and min(max(cg.halo(case.geom) - 1, 1), t) in case.lens
    assert sum(case.lens) < 2000 and cfg.len_mul <= 8
    assert case.ref.shape == (sum(case.row_lens), cfg.n_out)
    assert float(case.ref.abs().max()) > 0


def test_tables_cover_what_they_claim():
    assert {c.len_mul for c in cg.CONFIGS} == {1, 2, 8} and {c.n_in for c in cg.CONFIGS} == {1, 2, 3}
    assert {c.c_in for c in cg.CONFIGS} == {64, 192} and {c.n_out for c in cg.CONFIGS} == {32, 72, 160, 288}
    assert {c.in_scale for c in cg.CONFIGS} == {1.0, 0.5, 0.25} and {c.slope for c in cg.CONFIGS} == {None, 0.5, 0.25}
    assert {c.act for c in cg.CONFIGS} == {None, "relu"}
    assert any(c.x_window and c.n_in == 3 for c in cg.CONFIGS) and any(c.out_window for c in cg.CONFIGS)
    assert any(c.n_in > 1 and c.len_mul > 1 and c.slope for c in cg.CONFIGS)       # the HiFi-GAN upsampling launch
    assert {t for c in cg.CONFIGS for t in (c.tile,)} == {32, 64, 128}
    assert len(set(cg.GEOMS)) == 11 and all(0 <= p <= (k - 1) * d for k, d, p in cg.GEOMS)
    assert {g[0] for g in cg.WGRAD_GEOMS} == {1, 2, 3, 4, 5, 7}
    for (a, b) in cg.POLY_CHAINS:
        assert a in cg.POLYPHASE and b in cg.POLYPHASE
    assert {a for a, _ in cg.POLY_CHAINS} == set(cg.POLYPHASE) == {b for _, b in cg.POLY_CHAINS}


def test_folded_stride2_conv_equals_the_strided_conv():
    g = cg._gen("fold")
    for C0, pair_lens in ((64, [1, 2, 31, 32, 33, 150]), (96, [5, 1, 64])):
        wd = torch.randn(C0, C0, 3, generator=g, dtype=torch.float64)
        b = torch.randn(C0, generator=g, dtype=torch.float64)
        x = torch.randn(2 * sum(pair_lens), C0, generator=g, dtype=torch.float64)
        want = cg.reference_stride2(x, wd, b, pair_lens)
        got = cg.reference_conv(x.view(-1, 2 * C0), cg.fold_stride2(wd), b, pair_lens, 2, 1, 1)
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for C0 in cg.STRIDE2_CHANNELS:       # the integer cases of the GPU test: exact, operands and result inside f16
        case = cg.stride2_case(C0)
        assert _is_int(case.x) and _is_int(case.wd) and _is_int(case.b) and _is_int(case.ref) and float(case.ref.abs().max()) < cg.F16_EXACT
        assert float(case.x.abs().max()) * float(case.wd.abs().sum((1, 2)).max()) + float(case.b.abs().max()) < cg.F24
        assert torch.equal(cg.reference_conv(case.x.view(-1, 2 * C0), cg.fold_stride2(case.wd), case.b, cg.STRIDE2_PAIR_LENS, 2, 1, 1), case.ref)


@pytest.mark.parametrize("chain", range(len(cg.POLY_CHAINS)), ids=cg.POLY_CHAIN_IDS)
def test_polyphase_chain_equals_conv_transpose(chain):
    """hip.convtranspose_as_conv's promise, from the definition: the stride-1 conv's row j viewed as [s][c_out] is output steps j s .. j s + s - 1;
    the second stage runs on those rows at len_mul = s1.  Real-valued in float64, then the integer case of the GPU test (exactly)."""
    from jatts_amd import hip
    (s1, K1), (s2, K2) = cg.POLY_CHAINS[chain]
    case = cg.poly_case(chain)
    g = cg._gen("polyreal", chain)
    real = [(torch.randn(w.shape, generator=g, dtype=torch.float64), torch.randn(b.shape, generator=g, dtype=torch.float64), s) for w, b, s in case.stages]
    xr = torch.randn(case.x.shape, generator=g, dtype=torch.float64)
    for x, stages, tol in ((xr, real, 1e-12), (case.x.double(), case.stages, 0.0)):
        h, lens = x, list(cg.POLY_LENS)
        for w, b, s in stages:
            wc, pad = hip.convtranspose_as_conv(w.double(), s, cg.poly_padding(s))
            taps = wc.shape[-1]
            assert 0 <= pad <= taps - 1                          # inside jatts_conv1d's documented range
            h = cg.reference_conv(h, wc, b.double().repeat(s), lens, taps, 1, pad).reshape(-1, w.shape[1])
            lens = [v * s for v in lens]
        want = cg.reference_polyphase(x, stages, cg.POLY_LENS)
        assert h.shape == want.shape == (sum(cg.POLY_LENS) * s1 * s2, cg.POLY_CHANNELS[2])
        assert float((h - want).abs().max()) <= tol * float(want.abs().max())
    # the integer case is exact in every arithmetic: the intermediate is an f16 number, no partial sum of either stage reaches 2**24
    assert _is_int(case.mid) and float(case.mid.abs().max()) < cg.F16_EXACT and _is_int(case.ref) and float(case.ref.abs().max()) < cg.F16_EXACT
    (w1, b1, _), (w2, b2, _) = case.stages
    bound1 = float(case.x.abs().max()) * float(w1.abs().sum((0, 2)).max()) + float(b1.abs().max())
    bound2 = float(case.mid.abs().max()) * float(w2.abs().sum((0, 2)).max()) + float(b2.abs().max())
    assert bound1 < cg.F24 and bound2 < cg.F24


@pytest.mark.parametrize("si", range(len(cg.WGRAD_SHAPES)))
@pytest.mark.parametrize("gi", range(len(cg.WGRAD_GEOMS)), ids=[f"k{k}d{d}p{p}" for k, d, p in cg.WGRAD_GEOMS])
def test_wgrad_cases_are_exact_and_match_autograd(gi, si):
    for len_mul in (1, 4):
        case = cg.wgrad_case(gi, si, len_mul)
        k, dil, pad = case.geom
        assert _is_int(case.x) and _is_int(case.dy) and float(case.x.abs().max()) <= 8 and float(case.dy.abs().max()) <= 4
        assert float(case.x.abs().max()) * float(case.dy.abs().max()) * sum(case.row_lens) < cg.F24
        assert _is_int(case.dw) and _is_int(case.db)
        # the definition against float64 autograd through the explicitly padded conv
        w = torch.zeros(case.dy.shape[1], case.x.shape[1], k, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(case.dy.shape[1], dtype=torch.float64, requires_grad=True)
        cg.reference_conv(case.x, w, b, case.row_lens, k, dil, pad).backward(case.dy.double())
        assert torch.equal(w.grad, case.dw) and torch.equal(b.grad, case.db)


SENSITIVE = [(gi, 0) for gi in range(len(cg.GEOMS))] + [(0, 3), (2, 3), (9, 3)]        # every geometry at len_mul 1, three of them at len_mul 8


@pytest.mark.parametrize("gi,ci", SENSITIVE, ids=[f"{cg.GEOM_IDS[g]}-{cg.CONFIG_IDS[c]}" for g, c in SENSITIVE])
def test_comparison_rejects_one_row_geometry_errors(gi, ci):
    """check_exact -- the comparison of the GPU tests -- accepts the reference rounded to f32 and to f16 and REJECTS a result computed with a pad
    that is off by one, with a time tile's right halo dropped, and with a halo that reads the neighbouring utterance -- at len_mul 1 and 8."""
    case = cg.forward_case(gi, ci)
    k, dil, pad = case.geom
    cg.check_exact(case.ref.float(), case.ref)
    cg.check_exact(case.ref.half(), case.ref)
    faults = ["pad_off_by_one", "cross_utterance"] + (["no_right_halo"] if pad < (k - 1) * dil else [])
    for fault in faults:
        wrong = cg.reference_conv(case.u, case.w, case.b, case.row_lens, k, dil, pad, case.cfg.act, fault=fault)
        n_rows = int((wrong != case.ref).any(1).sum())
        assert n_rows > 0
        if fault != "pad_off_by_one":      # an edge fault: a few rows per utterance / tile out of hundreds -- what a model golden's tolerance absorbs
            assert n_rows <= (k - 1) * dil * (len(case.lens) + sum(case.row_lens) // 32)
        for dt in (torch.float32, torch.float16):
            with pytest.raises(AssertionError, match="differ from the integer reference"):
                cg.check_exact(wrong.to(dt), case.ref, fault)
    # ... and a single element, a NaN and a shape
    one = case.ref.float().clone()
    one[-1, -1] += 1
    nan = case.ref.float().clone()
    nan[0, 0] = float("nan")
    for bad in (one, nan, case.ref.float()[:-1]):
        with pytest.raises(AssertionError):
            cg.check_exact(bad, case.ref)


def test_entry_points_refuse_a_pad_outside_the_taps(lib):
    """include/jatts_hip.h: 0 <= pad <= (k_w - 1) dil.  The refusal comes from the argument checks, before anything is launched (the pointers here are
    host scratch that no kernel ever sees)."""
    from jatts_amd import _abi
    scratch = (C.c_float * 64)()
    p = C.addressof(scratch)
    for k, dil, pad, ok_pad in ((3, 1, -1, 0), (3, 1, 3, 2), (2, 1, 2, 1), (5, 2, 9, 8), (1, 1, 1, 0)):
        d = _abi.ConvDesc()
        d.rg = _abi.Ragged(p, 1, 0, 1, 0, None)       # max_len 0: a well-formed descriptor returns JATTS_OK without a launch
        d.dtype, d.n_in, d.ldx, d.in_scale = _abi.F32, 1, 64, 1.0
        d.x[0], d.w, d.y = p, p, p
        d.c_in, d.n_out, d.k_w, d.dil, d.ldy, d.y_is_f32, d.alpha = 64, 32, k, dil, 32, 1, 1.0
        d.pad = ok_pad
        assert lib.jatts_conv1d(C.byref(d), None) == 0
        d.pad = pad
        assert lib.jatts_conv1d(C.byref(d), None) == -1 and b"pad must lie in" in lib.jatts_last_error()
        rg = _abi.Ragged(p, 1, 0, 1, 0, None)
        assert lib.jatts_conv1d_wgrad(C.byref(rg), p, 64, p, 32, 64, 32, k, dil, ok_pad, p, None, p, None, None) == 0
        assert lib.jatts_conv1d_wgrad(C.byref(rg), p, 64, p, 32, 64, 32, k, dil, pad, p, None, p, None, None) == -1
        assert b"pad must lie in" in lib.jatts_last_error()
        assert lib.jatts_conv1d_wgrad_emul(C.byref(rg), p, 64, p, 32, 64, 32, k, dil, ok_pad, _abi.F32E, p, None, p, None, None) == 0
        assert lib.jatts_conv1d_wgrad_emul(C.byref(rg), p, 64, p, 32, 64, 32, k, dil, pad, _abi.F32E, p, None, p, None, None) == -1
        assert b"conv1d_wgrad_emul: pad must lie in" in lib.jatts_last_error()
