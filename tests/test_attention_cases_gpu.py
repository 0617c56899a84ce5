"""jatts_relpos_attention over the case table of attention_cases.py: every instantiation, tile schedule, V^T load path, bias form, mask and edge.
Selection cases are held to out[i] = v[pi(i)] by torch.equal, arithmetic cases to the elementwise a-priori bound of attention_cases.Case.bound against
the float64 attention; every buffer holds NaN wherever the kernel has no business, and the output's slack still holds it, bit for bit, afterwards.
(test_attention_cases_cpu.py proves the table's preconditions; profiles/attention_cases.txt lists case -> branch.)  rowdot_kernel, which produces the
u . k term, is held to float64 on the models' fused buffer at the end."""
import ctypes as C

import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu


def _run(c, cuda, lib):
    """One case on the device -> (out buffer, (R, H, dk) view of it).  The cases with the plain output stride go through hip.relpos_attention's own
    allocation when they carry the models' fused Q / K buffer (the models' call, argument for argument); every other one gets an output with NaN slack
    through a descriptor filled here -- hip.relpos_attention does not expose `out`."""
    from jatts_amd import _abi, hip
    t = AC.tensors(c, cuda)
    rb = hip.RaggedBatch(c.lens, cuda)
    ldq, qc0, ldk, kc0 = c.qk_layout()
    _, ldvt, _ = c.vt_geometry()
    for name in ("q", "k", "vt_buf", "out"):
        assert t[name].data_ptr() % 64 == 0
    assert t["vt"].data_ptr() % 32 == c.vt_props(0)["ptr"]      # structural: the layout the case describes is the layout the kernel gets
    if c.qk == "fused" and c.ldo_extra == 0:
        out = hip.relpos_attention(rb, t["q"], ldq, t["k"], ldk, t["vt"], ldvt, t["g"], c.ldg, t["ku"], c.scale, c.H, c.dk, c.arith, q_col0=qc0,
                                   k_col0=kc0, rel_mode=c.rel_mode, rel_center=c.center, vt_col0=t["vt_col0"], kv_len=t["kv"])
        assert out.shape == (c.R, c.A) and out.dtype == AC.tdtype(c.arith)
        return None, out.view(c.R, c.H, c.dk)
    d = _abi.RelAttnDesc()
    d.rg = rb.struct()
    d.dtype, d.n_heads, d.d_k = c.arith, c.H, c.dk
    d.q, d.ldq = hip._ptr(t["q"], qc0), ldq
    d.k, d.ldk = hip._ptr(t["k"], kc0), ldk
    d.vt, d.ldvt = t["vt"].data_ptr(), ldvt
    d.g, d.ldg = hip._ptr(t["g"]), c.ldg
    d.ku = hip._ptr(t["ku"])
    d.scale = c.scale
    d.out, d.ldo = t["out"].data_ptr(), c.ldo
    d.rel_mode, d.rel_center = c.rel_mode, c.center
    d.vt_col0, d.kv_len = hip._ptr(t["vt_col0"]), hip._ptr(t["kv"])
    _abi.check(lib.jatts_relpos_attention(C.byref(d), hip._stream()), "jatts_relpos_attention")
    torch.cuda.synchronize()
    return t, AC.out_view(c, t["out"])


def _slack_untouched(c, t):
    """Every element of the output's buffer outside the (R, A) matrix holds the NaN it was filled with, bit for bit."""
    bits = torch.int16 if c.arith == AC.F16 else torch.int32
    got = t["out"].cpu().view(bits)[~t["covered"]["out"]]
    nan = torch.full((1,), AC.NAN, dtype=AC.tdtype(c.arith)).view(bits)
    return got.numel() >= 8 and torch.equal(got, nan.expand_as(got))


def _check(c, t, view):
    got = view.float().cpu()
    assert bool(torch.isfinite(got).all()), (c.id, AC.branch(c), "NaN or inf in the result: a masked-out element was used")
    rows = c.exact_rows()
    if c.exact:
        want = c.expected()
        if not torch.equal(got[rows], want[rows]):      # derived: one-hot softmax over exact integers
            bad = (got != want)[rows].nonzero()
            assert False, (c.id, AC.branch(c), int(bad.shape[0]), "of", int(rows.sum()) * c.A, "first (row, head, channel)", bad[0].tolist())
    if not c.exact or not bool(rows.all()):
        ratio = ((got.double() - c.ref["out"]).abs() / c.bound())[~rows if c.exact else slice(None)]
        worst = float(ratio.max()) if ratio.numel() else 0.0
        print("attention arith", c.id, AC.branch(c), "worst err / bound", f"{worst:.4f}")
        assert worst <= 1.0, (c.id, worst)      # derived: attention_cases' docstring
    if t is not None:
        assert _slack_untouched(c, t), c.id


@pytest.mark.parametrize("c", [c for c in AC.CASES if c.group != "alone"], ids=AC.case_id)
def test_attention_case(cuda, lib, c):
    t, view = _run(c, cuda, lib)
    try:
        _check(c, t, view)
    finally:
        AC.release(c)


@pytest.mark.parametrize("c", [c for c in AC.CASES if c.group == "alone"], ids=AC.case_id)
def test_attention_alone_equals_inside_the_batch(cuda, lib, c):
    """Key tiles start at the sequence's first key and the Q scale of the split arithmetic is per workgroup: a sequence's output does not depend on
    what else the batch holds, in any arithmetic, bit for bit."""
    t, view = _run(c, cuda, lib)
    try:
        _check(c, t, view)
        whole, o = view.cpu(), 0
        for b, T in enumerate(c.lens):
            one = c.alone(b)
            t1, v1 = _run(one, cuda, lib)
            assert _slack_untouched(one, t1)
            assert torch.equal(v1.cpu(), whole[o:o + T]), (c.id, b, T)
            o += T
    finally:
        AC.release(c)


@pytest.mark.parametrize("dk", [32, 96, 192])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_rowdot_on_the_fused_buffer(cuda, lib, dt, dk):
    """rowdot_kernel as the models call it: x = the K half of the fused (rows, 2A) projection buffer (col0 = A), H = 3, d_k with and without a tail
    in the 64-lane loop.  |out - ref| <= (d_k + 2) 2**-23 sum |x| |vec| against float64: d_k products and adds in f32, in any order (the f16 input is
    exact in f32)."""
    from jatts_amd import hip
    H, rows = 3, 37
    A = H * dk
    g = torch.Generator().manual_seed(dk)
    x = torch.randn(rows, A, generator=g).to(dt)
    vec = torch.randn(H, dk, generator=g)
    buf = torch.full((rows, 2 * A), AC.NAN, dtype=dt)
    buf[:, A:] = x
    out = hip.rowdot(buf.to(cuda), 2 * A, rows, H, dk, vec.to(cuda), col0=A).cpu()
    xs = x.double().view(rows, H, dk)
    ref, mag = torch.einsum("rhd,hd->rh", xs, vec.double()), torch.einsum("rhd,hd->rh", xs.abs(), vec.double().abs())
    assert out.shape == (rows, H) and bool(torch.isfinite(out).all())
    ratio = float(((out.double() - ref).abs() / ((dk + 2) * AC.U * mag)).max())
    print("rowdot", dt, dk, "worst err / bound", f"{ratio:.4f}")
    assert ratio <= 1.0, (dk, ratio)
