"""jatts_bgemm and jatts_bgemm_emul over the case table of bgemm_cases.py: every tile, load path, batch index and edge.  Integer cases are held
to the float64 product of the same integers by torch.equal, arithmetic cases to the elementwise a-priori bound of bgemm_cases.bound_factor; in
both, every element of the operands' and the output's buffers that the matrices do not cover holds NaN before the call, and the output's still
holds it, bit for bit, afterwards.  (test_bgemm_cases_cpu.py proves the table's preconditions; profiles/bgemm_cases.txt lists case -> branch.)"""
import pytest
import torch

import bgemm_cases as BC

pytestmark = pytest.mark.gpu


def _run(c, cuda, lib, tile=None):
    """One case on the device -> (C's whole buffer, C's view of the matrices)."""
    from jatts_amd import hip
    a_cpu, b_cpu = c.data
    _, a = BC.place(c.la, c.a_shape(), a_cpu, cuda)
    _, b = BC.place(c.lb, c.b_shape(), b_cpu, cuda)
    cbuf, cv = BC.place(c.lc, c.c_shape(), c.start() if c.acc else None, cuda)      # NaN where the call overwrites: C must not be read there
    # the layout the case describes is the layout the kernel gets (structural: bgemm_cases.branch reads the same numbers)
    for t, layout in ((a, c.la), (b, c.lb), (cv, c.lc)):
        assert t.data_ptr() % 16 == 4 * (layout.off % 4) and t.stride() == (layout.so, layout.si, layout.ld, 1), (c.id, layout)
    tile = c.tile if tile is None else tile
    if c.acc == 0:
        out = hip.bgemm(a[0] if c.la.dims3 else a, b[0] if c.lb.dims3 else b, trans_a=c.ta, trans_b=c.tb, alpha=c.alpha, out=cv,
                        dtype=hip.F32E if c.kernel == "emul" else hip.F32, _tile=tile)
        assert out.data_ptr() == cv.data_ptr()
    else:      # hip.bgemm always overwrites: the C entries
        args = (a.data_ptr(), c.la.so, c.la.si, c.la.ld, int(c.ta), b.data_ptr(), c.lb.so, c.lb.si, c.lb.ld, int(c.tb), cv.data_ptr(), c.lc.so, c.lc.si,
                c.lc.ld, c.O, c.I, c.m, c.n, c.k, c.alpha, 1)
        for _ in range(c.acc):
            rc = lib.jatts_bgemm_emul(*args, BC.F32E | tile << 8, None) if c.kernel == "emul" else lib.jatts_bgemm(*args, None)
            assert rc == 0, lib.jatts_last_error()
        torch.cuda.synchronize()
    return cbuf, cv


def _slack_untouched(c, cbuf):
    """Every element of C's buffer outside the matrices holds the NaN it was filled with, bit for bit."""
    numel = c.O * c.I * c.m * c.n
    if c.lc.key() == (0, c.I * c.m * c.n, c.m * c.n, c.n):      # contiguous: the slack is what place() appends
        got = cbuf[numel:].cpu().view(torch.int32)
        assert got.numel() == 8      # structural: place() appends 8 floats
    else:
        idx, size = BC.covered(c.lc, c.c_shape())
        slack = torch.ones(size, dtype=torch.bool)
        slack[idx] = False
        got = cbuf.cpu().view(torch.int32)[slack]
    return torch.equal(got, torch.full((1,), BC.NAN).view(torch.int32).expand_as(got))


def _check_arith(c, cv):
    got = cv.double().cpu()
    assert bool(torch.isfinite(got).all()), c.id
    ratio = float(((got - c.ref).abs() / c.bound()).max())
    print("bgemm arith", c.id, "worst err / bound", f"{ratio:.3f}")
    assert ratio <= 1.0, (c.id, ratio)      # derived: bgemm_cases.bound_factor


@pytest.mark.parametrize("c", [c for c in BC.CASES if c.group != "bits"], ids=BC.case_id)
def test_bgemm_case(cuda, lib, c):
    cbuf, cv = _run(c, cuda, lib)
    try:
        if c.exact:
            got, want = cv.cpu(), c.expected().float()
            assert bool(torch.isfinite(got).all()), (c.id, "NaN or inf in the result: a masked-out element was used")
            if not torch.equal(got, want):      # derived: integer exactness
                bad = (got != want).nonzero()
                assert False, (c.id, BC.branch(c), int(bad.shape[0]), "of", got.numel(), "first", bad[0].tolist(),
                               float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
        else:
            _check_arith(c, cv)
        assert _slack_untouched(c, cbuf), c.id
    finally:
        BC.release(c)


@pytest.mark.parametrize("form", BC.FORMS, ids=lambda f: "NT"[f[0]] + "NT"[f[1]])
def test_bgemm_emul_one_bit_pattern_per_output(cuda, lib, form):
    """bgemm.hip's header: the same instruction sequence per accumulator in every tile variant and load path, so an output's bits do not depend on which
    variant computed it.  K = 70 (three chunks), all four forced tiles on the 16-byte path and on the same values one float off alignment."""
    group = [c for c in BC.CASES if c.group == "bits" and (c.ta, c.tb) == form]
    assert len(group) == 8 and len({c.seed for c in group}) == 1 and {BC.branch(c)[1:5] for c in group} == {
        (w, 32, mf, v) for w, mf in ((1, 2), (2, 2), (3, 2), (3, 1)) for v in (False, True)}      # structural
    first = None
    for c in group:
        cbuf, cv = _run(c, cuda, lib)
        _check_arith(c, cv)
        assert _slack_untouched(c, cbuf)
        got = cv.cpu()
        if first is None:
            first = got
        assert torch.equal(got, first), (c.id, int((got != first).sum()))
        BC.release(c)


def test_bgemm_refusals(cuda, lib):
    """hip.bgemm's ValueErrors and the exact entry's argument errors.  ("launch too large" is not provoked: were that check wrong, the call would launch
    over memory the test does not own.)"""
    from jatts_amd import hip
    a, b = torch.ones(1, 2, 8, 8, device=cuda), torch.ones(1, 2, 8, 8, device=cuda)
    with pytest.raises(ValueError, match="f32 tensors"):
        hip.bgemm(a.half(), b)                                        # dtype
    with pytest.raises(ValueError, match="f32 tensors"):
        hip.bgemm(a[0, 0], b)                                         # dims
    with pytest.raises(ValueError, match="f32 tensors"):
        hip.bgemm(a, b.transpose(-1, -2))                             # non-unit last stride
    with pytest.raises(ValueError, match="batch dims differ"):
        hip.bgemm(a, torch.ones(1, 3, 8, 8, device=cuda))
    with pytest.raises(ValueError, match="batch dims differ"):
        hip.bgemm(a, torch.ones(2, 2, 8, 8, device=cuda))
    with pytest.raises(ValueError, match="contraction sizes differ"):
        hip.bgemm(a, torch.ones(1, 2, 9, 8, device=cuda))
    with pytest.raises(ValueError, match="contraction sizes differ"):
        hip.bgemm(a, b[:, :, :, :7], trans_a=True, trans_b=True)
    for out in (torch.empty(1, 2, 8, 9, device=cuda), torch.empty(2, 8, 8, device=cuda), torch.empty(1, 2, 8, 8, device=cuda).half(),
                torch.empty(1, 2, 8, 8), torch.empty(1, 2, 8, 16, device=cuda)[..., ::2]):
        with pytest.raises(ValueError, match="out must be"):          # shape, dims, dtype, device, row stride
            hip.bgemm(a, b, out=out)
    with pytest.raises(ValueError, match="F32E6"):
        hip.bgemm(a, b, dtype=hip.F32E6)
    c = torch.full((1, 2, 8, 8), BC.NAN, device=cuda)

    def call(pa, pb, pc, k=8, lda=8, n_inner=2):
        return lib.jatts_bgemm(pa, 128, 64, lda, 0, pb, 128, 64, 8, 0, pc, 128, 64, 8, 1, n_inner, 8, 8, k, 1.0, 0, None)
    for ptrs in ((None, b.data_ptr(), c.data_ptr()), (a.data_ptr(), None, c.data_ptr()), (a.data_ptr(), b.data_ptr(), None)):
        assert call(*ptrs) != 0 and b"bgemm: null pointer" in lib.jatts_last_error()
    for kw in (dict(k=0), dict(lda=0), dict(n_inner=0), dict(k=-1)):
        assert call(a.data_ptr(), b.data_ptr(), c.data_ptr(), **kw) != 0 and b"bgemm: bad geometry" in lib.jatts_last_error()
    torch.cuda.synchronize()
    assert bool(c.isnan().all())                                      # a refused call launches nothing
    assert call(a.data_ptr(), b.data_ptr(), c.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(c, torch.full_like(c, 8.0))
