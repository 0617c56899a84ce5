"""GPU: the kernels of csrc/rowwise.hip at every dispatch branch, tile boundary and grid-stride step (case table, references and bounds:
tests/rowwise_edge_cases.py; the CPU half, tests/test_rowwise_edges_cpu.py, proves which branch a case reaches).

Every comparison is elementwise, |y - ref64| <= tol + tol |ref64| (+ 2**-10 |ref64| for an f16 output) with tol = max(T_k, 4 err32), or exact
(torch.equal) for moves, gathers and the integer paths.  Nothing is masked except the near-tie durations of predictor_head."""
import ctypes as C

import pytest
import torch

import rowwise_edge_cases as RC
from rowwise_edge_cases import ERR_ARG, ERR_UNSUPPORTED, SENTINEL, dev, dt_of, hold, ragged, refused, same, tdt

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cid", RC.ids_of("layernorm"))
def test_layernorm(cuda, lib, cid, out16):
    """Contiguous through the wrapper, then ldx = ldy = dim + 8 through the C ABI: the padding columns of x hold 1e4 (a row sum that reads
    them is far off), those of y a sentinel that must survive."""
    from jatts_amd import hip
    c = RC.CASES[cid]
    p, in16 = c.p, c.p["in16"]
    x, gamma, beta = dev(c.x["x"], cuda, in16), dev(c.x["gamma"], cuda), dev(c.x["beta"], cuda)
    hold(c, "y", hip.layernorm(x, gamma, beta, dt_of(out16), eps=p["eps"]), out16)
    rows, dim, ld = p["rows"], p["dim"], p["dim"] + 8
    xs = torch.full((rows, ld), 1e4, dtype=tdt(in16), device=cuda)
    xs[:, :dim] = x
    ys = torch.full((rows, ld), SENTINEL, dtype=tdt(out16), device=cuda)
    rc = lib.jatts_layernorm(xs.data_ptr(), dt_of(in16), ld, ys.data_ptr(), dt_of(out16), ld, rows, dim, gamma.data_ptr(), beta.data_ptr(),
                             p["eps"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    hold(c, "y", ys[:, :dim], out16)
    assert bool((ys[:, dim:] == SENTINEL).all())


def test_layernorm_refuses_dim_above_2048(cuda, lib):
    from jatts_amd import hip
    p = RC.LN_REFUSED
    x = torch.zeros(p["rows"], p["dim"], device=cuda)
    with refused(ERR_UNSUPPORTED, "layernorm: dim > 2048"):
        hip.layernorm(x, x[0].clone(), x[0].clone(), hip.F32)


# ------------------------------------------------------------------------------------------------------------------------- affine + cast
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cid", RC.ids_of("affine_cast"))
def test_affine_cast(cuda, lib, cid, out16):
    from jatts_amd import hip
    c = RC.CASES[cid]
    y = hip.affine_cast(dev(c.x["x"], cuda), dt_of(out16), scale=dev(c.x["scale"], cuda), shift=dev(c.x["shift"], cuda), ldy=c.p["ldy"])
    hold(c, "y", y, out16)
    assert not y[:, c.p["dim"]:].any()                    # ldy > dim zero-fills: exact zeros


@pytest.mark.parametrize("out16", [False, True])
def test_affine_slice_leaves_its_neighbours(cuda, lib, out16):
    from jatts_amd import hip
    c = RC.CASES["affine_slice/cols"]
    p = c.p
    out = torch.full((p["rows"], p["out_ld"]), SENTINEL, dtype=tdt(out16), device=cuda)
    hip.affine_cast(dev(c.x["x"], cuda), dt_of(out16), scale=dev(c.x["scale"], cuda), shift=dev(c.x["shift"], cuda), x_col0=p["col0"],
                    dim=p["dim"], out=out, out_col0=p["out_col0"])
    lo, hi = p["out_col0"], p["out_col0"] + p["dim"]
    hold(c, "y", out[:, lo:hi], out16)
    assert bool((out[:, :lo] == SENTINEL).all()) and bool((out[:, hi:] == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------- GLU + depthwise + BN + Swish
@pytest.mark.parametrize("cid", RC.ids_of("glu_dwconv_bn_swish"))
def test_glu_dwconv_bn_swish(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p, f16 = c.p, c.p["in16"]
    y = hip.glu_dwconv_bn_swish(ragged(p["lens"], cuda), dev(c.x["x"], cuda, f16), p["C"], p["K"], dev(c.x["w"], cuda), dev(c.x["s"], cuda),
                                dev(c.x["t"], cuda), dt_of(f16))
    hold(c, "y", y, f16)


def test_glu_dwconv_refusals(cuda, lib):
    from jatts_amd import hip
    for want, p in RC.GLU_REFUSED.items():
        C_, K = p["C"], p["K"]
        x, w, s = torch.zeros(4, 2 * C_, device=cuda), torch.zeros(C_, K, device=cuda), torch.zeros(C_, device=cuda)
        with (refused(ERR_UNSUPPORTED, "kernel too wide") if want == "refused-lds" else refused(ERR_ARG, "k_w must be odd")):
            hip.glu_dwconv_bn_swish(ragged([4], cuda), x, C_, K, w, s, s, hip.F32)


# ------------------------------------------------------------------------------------------------------------------------ predictor head
@pytest.mark.parametrize("cid", RC.ids_of("predictor_head"))
def test_predictor_head(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    v, d = hip.predictor_head(dev(c.x["x"], cuda, c.p["in16"]), dev(c.x["w"], cuda), c.p["b"], want_duration=True, offset=c.p["offset"])
    hold(c, "v", v)
    # duration_predictor.py:87-90 on the kernel's own log-durations: bit-exact except within 1e-4 of a .5 boundary
    want, near = RC.durations_of(v.cpu(), c.p["offset"])
    assert d.dtype == torch.int64 and torch.equal(d.cpu()[~near], want[~near]) and int(d.min()) >= 0


# ------------------------------------------------------------------------------------------------- 128-thread channel loops (dim > 128)
@pytest.mark.parametrize("cid", RC.ids_of("variance_embed_add"))
def test_variance_embed_add(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    x = {k: dev(v, cuda) for k, v in c.x.items()}
    hold(c, "hs", hip.variance_embed_add(ragged(c.p["lens"], cuda), x["hs"], x["p"], x["wp"], x["bp"], x["e"], x["we"], x["be"]))


@pytest.mark.parametrize("cid", RC.ids_of("add_seq_vector"))
def test_add_seq_vector(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    hold(c, "hs", hip.add_seq_vector(ragged(c.p["lens"], cuda), dev(c.x["hs"], cuda), dev(c.x["vec"], cuda)))


@pytest.mark.parametrize("cid", RC.ids_of("gated_tanh_sigmoid"))
def test_gated_tanh_sigmoid(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    f16 = c.p["in16"]
    y = hip.gated_tanh_sigmoid(ragged(c.p["lens"], cuda), dev(c.x["x"], cuda, f16), dev(c.x["gseq"], cuda), c.p["dim"], dt_of(f16))
    hold(c, "y", y, f16)


@pytest.mark.parametrize("cid", RC.ids_of("embed_scale"))
def test_embed_scale(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    same(c, "y", hip.embed_scale(dev(c.x["ids"], cuda), dev(c.x["table"], cuda), c.p["scale"]))


# ----------------------------------------------------------------------------------------------------------------------- GroupNorm + Mish
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cid", RC.ids_of("groupnorm_mish"))
def test_groupnorm_mish(cuda, lib, cid, out16):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    y = hip.groupnorm_mish(ragged(p["lens"], cuda), dev(c.x["x"], cuda, p["in16"]), p["C"], p["G"], dev(c.x["gamma"], cuda), dev(c.x["beta"], cuda),
                           dt_of(out16), eps=p["eps"], addvec=dev(c.x["add"], cuda), time_split=p["time_split"])
    hold(c, "y", y, out16)


# ------------------------------------------------------------------------------------------------- SnakeBeta and the grid-capped loops
@pytest.mark.parametrize("cid", RC.ids_of("snakebeta"))
def test_snakebeta(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    f16 = c.p["in16"]
    hold(c, "y", hip.snakebeta(dev(c.x["x"], cuda, f16), dev(c.x["alpha"], cuda), dev(c.x["inv_beta"], cuda)), f16)


@pytest.mark.parametrize("cid", RC.ids_of("gaussian_sample"))
def test_gaussian_sample(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    hold(c, "z", hip.gaussian_sample(dev(c.x["stats"], cuda), dev(c.x["noise"], cuda), c.p["noise_scale"]))


@pytest.mark.parametrize("cid", RC.ids_of("flip_channels"))
def test_flip_channels(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    same(c, "y", hip.flip_channels(dev(c.x["x"], cuda)))


# ------------------------------------------------------------------------------------------------------ l2_normalize, cfm_mix, sq_err_sum
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cid", RC.ids_of("l2_normalize"))
def test_l2_normalize(cuda, lib, cid, out16):
    from jatts_amd import hip
    c = RC.CASES[cid]
    y = hip.l2_normalize(dev(c.x["x"], cuda), dt_of(out16), ldy=c.p["ldy"], eps=c.p["eps"])
    hold(c, "y", y, out16)
    assert not y[2].any() and not y[:, c.p["dim"]:].any()      # the all-zero row gives zeros (not NaN); ldy > dim zero-fills


@pytest.mark.parametrize("cid", RC.ids_of("cfm_mix"))
def test_cfm_mix(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    y, u = hip.cfm_mix(ragged(c.p["lens"], cuda), dev(c.x["x1"], cuda), dev(c.x["z"], cuda), dev(c.x["t"], cuda), c.p["sigma"])
    hold(c, "y", y)
    hold(c, "u", u)


@pytest.mark.parametrize("cid", RC.ids_of("sq_err_sum"))
def test_sq_err_sum(cuda, lib, cid):
    """Within 1 ulp of the float64 sum rounded to f32, and the same bits on a second call (fixed summation order)."""
    from jatts_amd import hip
    c = RC.CASES[cid]
    a, b = dev(c.x["a"], cuda), dev(c.x["b"], cuda)
    s1, s2 = hip.sq_err_sum(a, b, c.p["scale"]).cpu(), hip.sq_err_sum(a, b, c.p["scale"]).cpu()
    want = c.ref64["s"][0].float()
    ulp = torch.nextafter(want, torch.tensor(float("inf"))) - want
    print(f"{c.id}: got {float(s1):.9e} want {float(want):.9e} ulp {float(ulp):.2e}")
    assert float((s1 - want).abs()) <= float(ulp) and torch.equal(s1, s2)


# --------------------------------------------------------------------------------------------------------------------- length regulator
@pytest.mark.parametrize("cid", RC.ids_of("lr_durations"))
def test_length_regulator(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    rb = ragged(p["lens"], cuda)
    d_eff, cum, olens, fb = hip.lr_durations(rb, dev(c.x["d"], cuda), p["alpha"], zero_rule=p["zero_rule"])
    same(c, "d_eff", d_eff)
    same(c, "cum", cum)
    same(c, "olens", olens)
    if p["zero_rule"] == 2:
        same(c, "fallback", fb)
    rbo = ragged([n + e for n, e in zip(c.r32["olens"].tolist(), p["extra"])], cuda)     # an output batch longer than sum(d): zero rows, index -1
    out, idx = hip.lr_gather(rb, cum, rbo, dev(c.x["x"], cuda), want_index=True)
    same(c, "out", out)
    same(c, "index", idx)


# ------------------------------------------------------------------------------------------------------------------------ zero_pad_rows
@pytest.mark.parametrize("cid", RC.ids_of("zero_pad_rows"))
def test_zero_pad_rows(cuda, lib, cid):
    """Rows t >= valid[b] become zero, every other element keeps its bits; with len_mul = 2 sequence b owns rows cu[b] * 2 .. cu[b+1] * 2 - 1
    and valid counts those rows (include/jatts_hip.h)."""
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    x = dev(c.x["x"], cuda, p["in16"])
    valid = torch.tensor(p["valid"], dtype=torch.int32, device=cuda)
    same(c, "x", hip.zero_pad_rows(ragged(p["lens"], cuda), x, valid, len_mul=p["mul"]))


# -------------------------------------------------------------------------------------------------------------------- gaussian upsample
@pytest.mark.parametrize("cid", RC.ids_of("gaussian_upsample"))
def test_gaussian_upsample(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    y = hip.gaussian_upsample(ragged(c.p["lens"], cuda), dev(c.x["d"], cuda), ragged(RC.gu_olens(c), cuda), dev(c.x["hs"], cuda), c.p["delta"])
    hold(c, "y", y)


def test_gaussian_upsample_refuses_a_text_above_16384(cuda, lib):
    from jatts_amd import hip
    p = RC.GU_REFUSED
    n = p["lens"][0]
    with refused(ERR_UNSUPPORTED, "text too long"):
        hip.gaussian_upsample(ragged(p["lens"], cuda), torch.ones(n, dtype=torch.int64, device=cuda), ragged([4], cuda),
                              torch.zeros(n, p["dim"], device=cuda))


# ----------------------------------------------------------------------------------------------------------------- HiFi-GAN output conv
@pytest.mark.parametrize("cid", RC.ids_of("hifigan_output"))
def test_hifigan_output(cuda, lib, cid):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p, f16 = c.p, c.p["in16"]
    xs = [dev(c.x[f"x{i}"], cuda, f16) for i in range(p["n_in"])]
    y = hip.hifigan_output(ragged(p["lens"], cuda), p["mul"], xs, p["in_scale"], p["slope"], p["C"], p["K"], dev(c.x["w"], cuda), p["bias"], dt_of(f16))
    hold(c, "y", y)


def test_hifigan_output_refuses_what_the_lds_cannot_hold(cuda, lib):
    from jatts_amd import hip
    p = RC.HO_REFUSED
    x = torch.zeros(16, p["C"], device=cuda)
    with refused(ERR_UNSUPPORTED, "c_in\\*k_w too large"):
        hip.hifigan_output(ragged([16], cuda), 1, [x], 1.0, 0.1, p["C"], p["K"], torch.zeros(p["K"], p["C"], device=cuda), 0.0, hip.F32)
