"""GPU: every store path of jatts_conv1d, exactly -- tight / windowed / transposed / two-output placements, every residual form (tight, windows, in place,
the half-row in-place window of the VITS flow), alpha, ragged and narrow n_out, the epilogue activations, and the geometries the exact input-side table
never reached (k_w = 1, reflect padding, halos beyond 32 rows) -- in every arithmetic, kernel and forced tile.

Integer cases (tests/conv_store_cases.py; preconditions, path coverage and sensitivity proven in tests/test_conv_store_cpu.py): the float64 value of the
definition is the expected content of the WHOLE output buffer bit for bit.  Every buffer is prefilled -- NaN, or the residual data of an in-place update --
so a store outside the window, a stale slack column of a V^T layout, a residual read from a neighbouring column or an unwritten element fails like a wrong
value.  tanh / swish / mish / SnakeBeta act on the same exact pre-activation and are held to the elementwise rule of tests/rowwise_edge_cases.py
(tol = max(T_k, 4 err32), an f16 store adds 2**-10 |ref|).  profiles/r35_notes.md: kernel -> case -> path, measured errors."""
import pytest
import torch

import conv_store_cases as cs
import test_conv_geometry_gpu as geo          # _weights / _variants / _conv: one arithmetic = operand type, packed weight, launch variants

pytestmark = pytest.mark.gpu


def _kernels(arith):
    """[(label, w_layout, launch kwargs)]: every kernel / forced tile of the arithmetic, plus the F32 register-streamed ring-4 kernel (variant 4)."""
    return geo._variants(arith, every_tile=True) + ([("v4", 0, dict(variant=4))] if arith == "F32" else [])


def _prepared(hip, arith, w):
    """The PreparedWeight forms of a split / emulated arithmetic ({w_layout: kwargs}): call sites say dtype=F32 and hip.conv1d picks the kernel."""
    if arith == "F32S":
        return {0: dict(w_packed=hip.SplitWeight(w, 64), dtype=hip.F32)}
    return {layout: dict(w_packed=hip.EmulWeight(w, 64, getattr(hip, arith), layout), dtype=hip.F32) for layout in (0, 1)}


def _launch_kwargs(hip, cuda, case, d, L, rb):
    k, dil, pad = case.geom
    kw = dict(dil=dil, pad=pad, bias=d.b.to(cuda), alpha=case.alpha, len_mul=case.len_mul, reflect=case.reflect, resid_col0=L.resid_col0)
    if case.act == "snake":
        kw["snake"] = tuple(v.to(cuda).contiguous() for v in d.snake)
    elif case.act:
        kw["act"] = {"relu": hip.ACT_RELU, "tanh": hip.ACT_TANH, "swish": hip.ACT_SWISH, "mish": hip.ACT_MISH}[case.act]
    col0, ld = cs.seq_col0(case)
    vcol = None
    if col0 is not None:
        vcol = torch.tensor(col0, dtype=torch.int32, device=cuda)
        if case.tr == "vt" or case.split:          # the layout under test IS RaggedBatch.vt_layout
            lib_col, lib_ld = rb.vt_layout()
            assert lib_col.cpu().tolist() == col0 and lib_ld * case.len_mul == ld
    if case.tr:
        kw.update(transposed=True, y_seq_col0=vcol)
    else:
        kw.update(out_ld=L.out_ld, out_col0=L.out_col0)
    if case.split:
        kw["split"] = (case.split, ld, vcol)
    return kw


def _run_case(hip, cuda, arith, case, figures):
    """Every kernel of `arith` on one case: the whole output buffer(s) against the expectation."""
    from jatts_amd._abi import JattsHipError
    half = arith == "F16"
    d, L, exp = cs.data(case.name), cs.layout(case), cs.expected(case.name)
    nonlinear = case.act in cs.NONLINEAR
    rb = hip.RaggedBatch(case.lens, cuda)
    x = [t.to(torch.float16 if half else torch.float32).to(cuda) for t in d.xs]
    wdev = d.w.to(cuda)
    kw = _launch_kwargs(hip, cuda, case, d, L, rb)
    resid = d.rbuf.float().to(cuda) if L.resid_shape and not L.alias else None
    forms = [("", geo._weights(hip, arith, wdev))]
    if cs.wide_halo(case) and arith in ("F32S", "F32E", "F32E6"):
        # beyond the split / emulated staging: the raw dtype is refused (nothing launches), the PreparedWeight form takes the exact-f32 kernel
        forms = [("refused", forms[0][1]), ("prepared ", _prepared(hip, arith, wdev))]
    for form, wk in forms:
        for label, layout, vkw in _kernels(arith):
            y16 = half and not vkw.get("out_f32")
            odt = torch.float16 if y16 else torch.float32
            what = f"{arith} {form}{label} {case.name}"
            out = exp.out0.to(odt).to(cuda)
            out2 = exp.out2_0.to(odt).to(cuda) if case.split else None
            r = out if L.alias else resid
            if L.alias and y16:
                with pytest.raises(ValueError, match="residual must be f32"):        # an f16 y cannot be the f32 residual stream
                    geo._conv(hip, rb, x, wk[layout], case.c_in, case.n_out, case.geom[0], out=out, resid=r, **kw, **vkw)
                continue
            assert out.data_ptr() % 16 == 0 and (r is None or r.data_ptr() % 16 == 0), "the path model takes 16-byte aligned allocations"
            call = dict(out=(out, out2) if case.split else out, resid=r, **kw, **vkw)
            if form == "refused":
                with pytest.raises(JattsHipError):
                    geo._conv(hip, rb, x, wk[layout], case.c_in, case.n_out, case.geom[0], **call)
                continue
            got = geo._conv(hip, rb, x, wk[layout], case.c_in, case.n_out, case.geom[0], **call)
            assert (got[0] is out and got[1] is out2) if case.split else got is out
            allowed = None
            if nonlinear:
                err32, tol, a32, a16 = cs.bound(case.name)
                allowed = a16 if y16 else a32
            worst = cs.check_buffer(out, exp.want, what, None if allowed is None else allowed.want)
            if case.split:
                worst = max(worst, cs.check_buffer(out2, exp.want2, what + " (second output)", None if allowed is None else allowed.want2))
            if nonlinear:
                keep = ~torch.isnan(exp.want)
                dmax = float((out.cpu().double() - exp.want)[keep].abs().max())
                f = figures.setdefault((case.act, "f16 y" if y16 else "f32 y"), [0.0, 0.0, tol, err32])
                f[0], f[1], f[2], f[3] = max(f[0], dmax), max(f[1], worst), max(f[2], tol), max(f[3], err32)


@pytest.mark.parametrize("arith", cs.ARITHS)
@pytest.mark.parametrize("axis", cs.AXES)
def test_conv1d_store_paths(cuda, lib, axis, arith):
    """One store axis in one arithmetic: every case of the axis through every kernel and forced tile.  Exact cases: the whole buffer equals the integer
    reference (canaries included); non-linear activations: the elementwise bound on the exact pre-activation, figures printed per activation."""
    from jatts_amd import hip
    figures = {}
    for case in cs.of_axis(axis):
        _run_case(hip, cuda, arith, case, figures)
    for (act, store), (dmax, worst, tol, err32) in sorted(figures.items()):
        print(f"conv store {arith} {act} {store}: max |y - ref64| = {dmax:.3e}, worst |d| / allowed = {worst:.3f} (tol = {tol:.2e}, err32 = {err32:.2e})")


def test_two_output_buffers_argument_checks(cuda, lib):
    """split with the caller's own buffers, out=(out, out2): a single tensor, a second output that is too small or of another dtype, and a window that
    does not fit its row are refused on the host."""
    from jatts_amd import hip
    rb = hip.RaggedBatch([10], cuda)
    x = torch.zeros(10, 64, device=cuda)
    w = hip.pack_conv_weight(torch.zeros(264, 64, 1, device=cuda), hip.F32)
    vcol, ld2 = rb.vt_layout()
    out, out2 = torch.zeros(10, 280, device=cuda), torch.zeros(8, ld2, device=cuda)
    kw = dict(dtype=hip.F32, split=(256, ld2, vcol), out_ld=280, out_col0=8)
    got = hip.conv1d(rb, x, w, 64, 264, 1, out=(out, out2), **kw)
    assert got[0] is out and got[1] is out2
    for bad in (out, (out, out2[:7]), (out, out2.half()), (out[:9], out2)):
        with pytest.raises(ValueError):
            hip.conv1d(rb, x, w, 64, 264, 1, out=bad, **kw)
    with pytest.raises(ValueError):
        hip.conv1d(rb, x, w, 64, 264, 1, out=(out, out2), **dict(kw, out_col0=32))       # 32 + 256 > 280


@pytest.mark.parametrize("arith", cs.ARITHS)
def test_wrong_store_geometry_is_rejected_on_the_device(cuda, lib, arith):
    """The kernels themselves launched with a store geometry that is wrong by one thing -- the residual window four columns to the left, the V^T columns of
    another len_mul -- give buffers the comparison rejects; the right launch next to each is accepted."""
    from jatts_amd import hip
    half = arith == "F16"
    for name, wrong in (("r_win", dict(resid_col0=4)), ("t_seq2", dict(y_seq_col0="halved"))):
        case = cs.BY_NAME[name]
        d, L, exp = cs.data(name), cs.layout(case), cs.expected(name)
        rb = hip.RaggedBatch(case.lens, cuda)
        x = d.x.to(torch.float16 if half else torch.float32).to(cuda)
        wk = geo._weights(hip, arith, d.w.to(cuda))
        kw = _launch_kwargs(hip, cuda, case, d, L, rb)
        resid = d.rbuf.float().to(cuda) if L.resid_shape else None
        bad = dict(kw)
        if "y_seq_col0" in wrong:
            bad["y_seq_col0"] = kw["y_seq_col0"] // 2          # (still inside the buffer: every column moves to the left)
        else:
            bad.update(wrong)
        for label, layout, vkw in geo._variants(arith, every_tile=False):
            odt = torch.float16 if half and not vkw.get("out_f32") else torch.float32
            for kwargs, ok in ((kw, True), (bad, False)):
                out = exp.out0.to(odt).to(cuda)
                geo._conv(hip, rb, x, wk[layout], case.c_in, case.n_out, case.geom[0], out=out, resid=resid, **kwargs, **vkw)
                if ok:
                    cs.check_buffer(out, exp.want, f"{arith} {label} {name}")
                else:
                    with pytest.raises(AssertionError, match="differ from the integer reference|outside the output window|inside the output window"):
                        cs.check_buffer(out, exp.want, f"{arith} {label} {name} (wrong launch)")
