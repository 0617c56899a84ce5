"""GPU: every case of tests/resunit_cases.py through hip.hifigan_resunit (two convs) / hip.hifigan_resblock in every arithmetic it lists, against the
float64 reference WITHOUT a tolerance: the operands are dyadic numbers on which no arithmetic rounds (tests/test_resunit_cases_cpu.py proves it per
case), so the result is bit-equal after the one rounding of the store type -- one wrong tap at one window's last column, an h row beyond the
utterance's end left at lrelu(b1), a residual or halo row read from the neighbouring utterance each change it.

x, the MRF partners and y lie inside larger buffers with 16-byte-aligned margins: NaN around the inputs (a row read beyond the batch poisons the
result), a sentinel around and in y (the margins must stay untouched, every row of y must be written).  Per case and arithmetic three identities
hold bit for bit: the sliding form equals the windowed form (w_layout 1), the 1-D ragged grid equals the rectangular grid, and the first utterance
launched alone equals the same utterance inside the batch (another tile, where the launch size chooses it).  hip.resunit_variant reports the form
tile_of predicts for the w_layout 1 launches."""
import functools

import pytest
import torch

import resunit_cases as rc

pytestmark = pytest.mark.gpu

MARGIN = 64                 # elements: 128 B (f16) / 256 B (f32)
SENTINEL = -7776.0          # an f16 number no case produces


def _code(hip, spec):
    return getattr(hip, rc.SPECS[spec][0])


@functools.lru_cache(maxsize=8)
def _packed(name, recipe, spec):
    """The case's weights in the operand form of `spec`, on the GPU: [(w1, b1, w2, b2, dil)], and the inverse scales of the split arithmetic."""
    from jatts_amd import hip
    dev = torch.device("cuda:0")
    code, w_layout, _ = rc.SPECS[spec]
    units, ws = [], []
    for w1, b1, w2, b2, dil in rc.inputs(name, recipe).units:
        ps = []
        for w in (w1.to(dev), w2.to(dev)):
            if code == "F32S":
                ps.append(hip.pack_conv_weight_split(w, 32))
            elif code in ("F32E", "F32E6"):
                ps.append((hip.pack_unit_weight_bf16x3_k32(w) if w_layout == 1 else hip.pack_conv_weight_bf16x3(w, 32), None))
            else:
                ps.append((hip.pack_conv_weight(w, getattr(hip, code), 32), None))
        units.append((ps[0][0], b1.to(dev), ps[1][0], b2.to(dev), dil))
        ws.append((ps[0][1], ps[1][1]))
    return units, ws


def _framed(t, fill, dtype, dev):
    """-> (buffer, view): `t` inside a buffer with MARGIN elements of `fill` on either side."""
    n = t.numel()
    buf = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=dev)
    view = buf[MARGIN:MARGIN + n].view(t.shape)
    view.copy_(t.to(dev))
    assert view.data_ptr() % 16 == 0
    return buf, view


def _launch(hip, dev, case, spec, d, packed, lens, rows, variant=0):
    """One launch over the first `rows` rows (the utterances `lens`) -> y; asserts that the margins of y are untouched."""
    code = _code(hip, spec)
    tdt = hip.torch_dtype(code)
    units, ws = packed
    _, x = _framed(d.x[:rows], float("nan"), tdt, dev)
    adds = [_framed(a[:rows], float("nan"), tdt, dev)[1] for a in d.adds] or None
    ybuf, y = _framed(torch.full((rows, case.C), SENTINEL), SENTINEL, tdt, dev)
    rb = hip.RaggedBatch(lens, dev)
    if case.form == "unit":
        w1, b1, w2, b2, dil = units[0]
        hip.hifigan_resunit(rb, case.len_mul, x, y, w1, b1, w2, b2, case.C, case.k, dil, d.slope, code, add=adds, out_scale=case.out_scale,
                            ws=ws[0] if code == hip.F32S else None, w_layout=rc.SPECS[spec][1], variant=variant)
    else:
        hip.hifigan_resblock(rb, case.len_mul, x, y, units, case.C, case.k, d.slope, code, add=adds, out_scale=case.out_scale,
                             ws=ws if code == hip.F32S else None)
    torch.cuda.synchronize()
    assert bool((ybuf[:MARGIN] == SENTINEL).all()) and bool((ybuf[-MARGIN:] == SENTINEL).all()), "wrote outside y"
    return y


PARAMS = [pytest.param(c.name, s, id=f"{c.name}-{s}") for c in rc.CASES for s in c.specs]


@pytest.mark.parametrize("name,spec", PARAMS)
def test_case_is_exact(cuda, lib, monkeypatch, name, spec):
    from jatts_amd import hip
    case = rc.CASE_BY_NAME[name]
    d = rc.inputs(name, rc.recipe_of(case, spec))
    packed = _packed(name, rc.recipe_of(case, spec), spec)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    lens, rows = d.lens, sum(d.row_lens)
    w1 = rc.SPECS[spec][1] == 1
    t = rc.case_tile(name, spec, 1 if w1 else 0, cus)
    y = _launch(hip, cuda, case, spec, d, packed, lens, rows, variant=1 if w1 else 0)
    rc.check_exact(y, d.ref, f"{name} {spec} <{t.args}>")
    if w1:      # the sliding form and the library's own choice; the form reported is the model's
        for variant in (2, 0):
            yv = _launch(hip, cuda, case, spec, d, packed, lens, rows, variant=variant)
            assert torch.equal(yv, y), f"{name} {spec}: variant {variant} != windowed at {int((yv != y).sum())} elements"
        units, _ = packed
        p1, b1, p2, b2, dil = units[0]
        rb = hip.RaggedBatch(lens, cuda)
        for variant in (0, 1, 2):
            want = 2 if rc.case_tile(name, spec, variant, cus).sliding else 1
            got = hip.resunit_variant(rb, case.len_mul, y, torch.empty_like(y), p1, b1, p2, b2, case.C, case.k, dil, d.slope, _code(hip, spec), w_layout=1,
                                      variant=variant)
            assert got == want, f"{name} {spec} variant {variant}: the library reports form {got}, the model {want}"
    # the first utterance alone (the launch-size cases: on the small-launch tile)
    n0 = d.row_lens[0]
    y0 = _launch(hip, cuda, case, spec, d, packed, lens[:1], n0, variant=1 if w1 else 0)
    assert torch.equal(y0, y[:n0]), f"{name} {spec}: the first utterance alone differs at {int((y0 != y[:n0]).sum())} elements"
    # the rectangular grid (windows of the longest utterance x utterances) against the 1-D grid over the real windows
    assert hip.RaggedBatch(lens, cuda).struct(case.len_mul).total_rows > 0
    monkeypatch.setattr(hip, "_RAGGED_1D", False)
    assert hip.RaggedBatch(lens, cuda).struct(case.len_mul).total_rows == 0
    yr = _launch(hip, cuda, case, spec, d, packed, lens, rows, variant=1 if w1 else 0)
    assert torch.equal(yr, y), f"{name} {spec}: the rectangular grid differs at {int((yr != y).sum())} elements"
    if w1:
        ys = _launch(hip, cuda, case, spec, d, packed, lens, rows, variant=2)
        assert torch.equal(ys, y), f"{name} {spec}: sliding over the rectangular geometry differs at {int((ys != y).sum())} elements"


WRONG = [pytest.param(n, s, id=f"{n}-{s}") for n in ("u64-k7-d1", "u128-k11-d5", "u256-k7-d5") for s in rc.CASE_BY_NAME[n].specs]


@pytest.mark.parametrize("name,spec", WRONG)
def test_a_merged_batch_is_rejected_on_the_device(cuda, lib, name, spec):
    """Sensitivity on the device: the same rows launched as ONE utterance (every halo reads its neighbours) are rejected by check_exact against the
    case's reference, and equal the reference's own "cross_utterance" fault bit for bit (operands 8 bits wide: exact there as well)."""
    from jatts_amd import hip
    case = rc.CASE_BY_NAME[name]
    recipe = rc.recipe_of(case, spec)
    d = rc.inputs(name, recipe)
    rows = sum(d.row_lens)
    y = _launch(hip, cuda, case, spec, d, _packed(name, recipe, spec), [sum(d.lens)], rows, variant=0)
    with pytest.raises(AssertionError, match="differ from the integer reference"):
        rc.check_exact(y, d.ref, name)
    rc.check_exact(y, rc.reference_fault(name, recipe, "cross_utterance"), f"{name} {spec} merged")
