"""CPU: the case table of the two-conv fused units and ResBlocks (tests/resunit_cases.py) does what tests/test_resunit_cases_gpu.py relies on --
the dispatcher model names exactly the instantiations of the sources, the table launches every one of them, every case is exact in every
arithmetic it runs under (proven from the reference's own float64 intermediates), every weight column is observable, every fault a kernel could
have changes the expected output at the rows it should, and the reference agrees with a plain F.conv1d / F.leaky_relu chain."""
import pytest
import torch
import torch.nn.functional as F

import resunit_cases as rc

CASE_IDS = [c.name for c in rc.CASES]
CASE_RECIPES = [(c.name, r) for c in rc.CASES for r in sorted({rc.recipe_of(c, s) for s in c.specs})]


def test_model_names_the_instantiations_of_the_sources():
    """The `launch_*<...>` template-argument lists of the nine dispatcher files are the model's, file by file: a tile added to or removed from a
    dispatcher fails here until tile_of (and then the table) follows."""
    src = rc.source_instantiations()
    model = {(k[2], k[3], k[4]) for k in rc.model_instantiations()}
    assert len(src) >= 40
    assert src == model, f"only in the sources: {sorted(src - model)}; only in the model: {sorted(model - src)}"


@pytest.mark.parametrize("cus", [rc.CUS, 64])
def test_table_reaches_every_instantiation(cus):
    """Every (form, arithmetic spec, instantiation, windowed / sliding) tile_of can return is launched by a case, at the MI355X's CU count and at a
    smaller one (the sliding pick's runs = CUs x workgroups per CU; the w_layout 0 rules count workgroups, not CUs)."""
    model = rc.model_instantiations(cus)
    reach = rc.reached(cus)
    assert set(reach) == model, f"not launched: {sorted(model - set(reach))}; not in the model: {sorted(set(reach) - model)}"


def test_launch_size_branches_by_arithmetic():
    """The launch-size cases cross their rules by the dispatchers' own arithmetic: the rectangular workgroup count of the w_layout 0 windows, and
    positions >= 2 x runs x WGCOLS for the sliding pick -- which flips with the CU count."""
    for name, win, thr in (("u128-k3-d1-wgs", 128, 448), ("u256-k3-d1-wgs", 64, 160), ("u256-k3-d21-wgs", 64, 160)):
        case = rc.CASE_BY_NAME[name]
        lens = rc.lens_of(name)
        tt = win - (case.k - 1)
        wgs = -(-max(lens) // tt) * len(lens)
        assert wgs > thr and -(-max(lens) // tt) * (len(lens) - 1) <= thr, (name, wgs)        # the smallest batch of these lengths beyond the rule
        for spec in case.specs:
            big, one = rc.case_tile(name, spec), rc.case_tile(name, spec, lens=lens[:1])
            assert big.wgcols == win and one.wgcols == win // 2, (name, big, one)
    small = rc.case_tile("u256-k3-d1-small", "e7w0")
    assert small.wgcols == 32
    assert rc.case_tile("u256-k11-d5", "e7w0").args.endswith("true") and rc.case_tile("u256-k3-d21-wgs", "e7w0").args.endswith("true")   # channel halves
    name = "u128-k3-d1-auto"
    positions = sum(rc.lens_of(name))
    for cus in (rc.CUS, 64, 304):
        t = rc.case_tile(name, "e7w1", 0, cus)
        assert t.sliding == (positions >= 2 * cus * 1 * 128), (cus, t)
    assert rc.case_tile(name, "e7w1", 0, rc.CUS).sliding and not rc.case_tile(name, "e7w1", 0, 304).sliding
    assert not rc.case_tile(name, "e7w1", 1).sliding and rc.case_tile(name, "e7w1", 2).sliding
    # the residual-register tiles (C <= 64) slide only when forced; a sliding tail beyond 160 KiB stays windowed even then
    assert not rc.case_tile("u64-k7-d1", "e7w1", 0, 1).sliding and rc.case_tile("u64-k7-d1", "e7w1", 2).sliding
    assert not rc.case_tile("u256-k11-d4", "e7w1", 2).sliding and rc.case_tile("u256-k7-d5", "e7w1", 2).sliding


def test_refusals_of_the_model():
    """Shapes the library refuses have no tile: channel counts without a kernel, a halo beyond the one-batch staging, receptive fields too wide."""
    assert rc.tile_of("unit", "f32", 0, 0, 512, 3, 1, 1, 8, 0, 1) is None
    assert rc.tile_of("unit", "f32s", 0, 0, 64, 7, 12, 1, 8, 0, 1) is None                 # 2 p1 = 72 > 64
    assert rc.tile_of("unit", "e7", 1, 0, 256, 7, 12, 1, 8, 0, 1) is None                  # channel halves: 2 p1 = 72 > 64
    assert rc.tile_of("unit", "f32", 1, 0, 64, 3, 1, 1, 8, 0, 1) is None                   # w_layout 1 is the emulated units'
    assert rc.tile_of("block", "f32", 0, 0, 64, 7, (1, 3, 5), 1, 8, 0, 1) is None          # 2 H = 72 > 32
    assert rc.tile_of("block", "e7", 0, 0, 64, 11, (1, 3, 5), 1, 8, 0, 1) is None          # tt_out = 8 < 32
    assert rc.tile_of("block", "f16", 0, 0, 256, 3, (1, 3, 5), 1, 8, 0, 1) is None
    t = rc.tile_of("block", "f16", 0, 0, 64, 7, (1, 3, 5), 1, 8, 0, 1)
    assert (t.wgcols, t.tt_out) == (512, 512 - 72)                                          # H = sum p2 (dil + 1) = 36


@pytest.mark.parametrize("name", CASE_IDS)
def test_lengths_sit_on_every_launched_window(name):
    """Each case holds tt - 1, tt, tt + 1, 2 tt - 1, 2 tt, 2 tt + 1 (in positions; len_mul cases: the lengths that round up to them) of every window
    its specs launch, utterances of 1 and 2 rows and one below the per-side halo, each between two others of 20 rows or more (or its own length: a neighbour's
    rows lie inside every halo), and one of three windows or more."""
    case = rc.CASE_BY_NAME[name]
    lens = list(rc.lens_of(name))
    if case.kind in ("auto", "carry"):      # (one pattern of short and long utterances, repeated to the launch size)
        t = rc.case_tile(name, case.specs[0], 2)
        runs = rc.CUS * int(t.args.split(", ")[5])
        assert t.sliding and min(lens) == 1 and max(lens) > 3 * t.wgcols and sum(lens) >= (3 if case.kind == "carry" else 2) * runs * t.wgcols
        return
    pos = [v * case.len_mul for v in lens]
    for spec in case.specs:
        for variant in rc._variants(spec):
            t = rc.case_tile(name, spec, variant)
            tt = t.tt_out
            for e in (tt - 1, tt, tt + 1, 2 * tt - 1, 2 * tt, 2 * tt + 1):
                assert any(e <= p < e + case.len_mul for p in pos), (name, spec, tt, e)
            assert max(pos) > 3 * tt
    below = max(rc.side_halo(case) - 1, 1)
    for short in (1, 2, below):
        i = lens.index(short)
        assert 0 < i < len(lens) - 1 and min(lens[i - 1], lens[i + 1]) >= min(short, 20), (name, short)


@pytest.mark.parametrize("name", CASE_IDS)
def test_every_arithmetic_is_exact(name):
    """No case is exempt: the preconditions of every spec it runs under hold on the generated tensors and the reference's intermediates."""
    case = rc.CASE_BY_NAME[name]
    for spec in case.specs:
        m = rc.preconditions(name, spec)
        print(f"{name} {spec} ({rc.recipe_of(case, spec)}): max|a| {m['max_a']:g} max|g| {m['max_g']:g} max|y| {m['max_y']:g} max|out| {m['max_out']:g} "
              f"lsb 2^{m['lsb']} operand bits {m['bits']} partial sums <= {m['sum_units']:g} lsb units")


@pytest.mark.parametrize("name,recipe", CASE_RECIPES)
def test_every_weight_column_is_observable(name, recipe):
    """Exactly m non-zeros in every (c_in, tap) column and m k in every output channel's row, of every weight: a skipped tap or K-chunk shows."""
    case = rc.CASE_BY_NAME[name]
    for w1, b1, w2, b2, _ in rc.inputs(name, recipe).units:
        for w in (w1, w2):
            assert bool(((w != 0).sum(0) == case.m).all()) and bool(((w != 0).sum((1, 2)) == case.m * case.k).all())
        assert bool((b1 != 0).any()) and bool((b2 != 0).any())


def _dist_rows(row_lens):
    """Per row: its distance to the nearer end of its own utterance (0 for the first and last row), and the utterance's index."""
    dist, seq = [], []
    for i, L in enumerate(row_lens):
        r = torch.arange(L)
        dist.append(torch.minimum(r, L - 1 - r))
        seq.append(torch.full((L,), i))
    return torch.cat(dist), torch.cat(seq)


# (a conv2 at conv1's dilation is the same conv at dilation 1: the one fault that does not apply to every case)
FAULT_PARAMS = [(n, r, f) for n, r in CASE_RECIPES for f in rc.FAULTS if f != "dil_on_conv2" or max(rc.CASE_BY_NAME[n].dils) > 1]


@pytest.mark.parametrize("name,recipe,fault", FAULT_PARAMS)
def test_every_fault_changes_the_expected_output(name, recipe, fault):
    """The expected output moves under every fault, and only at the rows the fault reaches: within the per-side halo of an utterance's end (h not
    masked; the neighbour read: ends that have a neighbour), within it of a window boundary (a window reading zeros beyond its columns), and in most
    rows of the batch (no residual, a dilated conv2)."""
    case = rc.CASE_BY_NAME[name]
    d = rc.inputs(name, recipe)
    spec = next(s for s in case.specs if rc.recipe_of(case, s) == recipe)
    tt = rc.case_tile(name, spec, 1).tt_out
    bad = rc.reference_fault(name, recipe, fault, tt=tt)
    rows = (bad != d.ref).any(1)
    H = rc.side_halo(case)
    dist, seq = _dist_rows(d.row_lens)
    assert bool(rows.any()), f"{name}: {fault} leaves the expected output unchanged"
    if fault == "h_not_masked":
        named = dist < H
    elif fault == "cross_utterance":
        named = dist < H
        first, last = seq == 0, seq == len(d.row_lens) - 1
        assert int((rows & ~first & ~last).sum()) > 0
    elif fault == "window_halo_zero":
        o, named = 0, torch.zeros_like(rows)
        for L in d.row_lens:
            for t0 in range(tt, L, tt):
                named[o + max(t0 - H, 0):o + min(t0 + H, L)] = True
            o += L
    else:
        named = torch.ones_like(rows)
        assert int(rows.sum()) > rows.numel() // 2, f"{name}: {fault} changes only {int(rows.sum())} of {rows.numel()} rows"
    assert not bool((rows & ~named).any()), f"{name}: {fault} changes rows beyond its reach"
    print(f"{name} {recipe} {fault}: {int(rows.sum())} of {rows.numel()} rows change, first {rows.nonzero().view(-1)[:6].tolist()}")


def test_reference_agrees_with_the_library_chain():
    """One small case against F.conv1d(padding=) / F.leaky_relu applied utterance by utterance, and the MRF pass."""
    name = "b64-k3-add1"
    case = rc.CASE_BY_NAME[name]
    d = rc.inputs(name, "half")
    outs, o = [], 0
    for L in d.row_lens:
        x = d.x[o:o + L].double().t().unsqueeze(0)
        for w1, b1, w2, b2, dil in d.units:
            p2 = (case.k - 1) // 2
            h = F.conv1d(F.leaky_relu(x, d.slope), w1.double(), b1.double(), padding=p2 * dil, dilation=dil)
            x = x + F.conv1d(F.leaky_relu(h, d.slope), w2.double(), b2.double(), padding=p2)
        outs.append(x[0].t())
        o += L
    want = (torch.cat(outs) + d.adds[0].double()) * case.out_scale
    assert torch.equal(want, d.ref)
    name = "u128-k7-d5"
    case = rc.CASE_BY_NAME[name]
    d = rc.inputs(name, "half")
    w1, b1, w2, b2, dil = d.units[0]
    y = rc.reference_unit(d.x, w1, b1, w2, b2, d.row_lens, case.k, dil, d.slope)
    assert torch.equal(y, d.ref)
    L = d.row_lens[0]
    x = d.x[:L].double().t().unsqueeze(0)
    h = F.conv1d(F.leaky_relu(x, 0.5), w1.double(), b1.double(), padding=15, dilation=5)
    assert torch.equal((x + F.conv1d(F.leaky_relu(h, 0.5), w2.double(), b2.double(), padding=3))[0].t(), d.ref[:L])


def test_lsb_exp():
    assert rc.lsb_exp(torch.tensor([3.0, 0.0, -6.0], dtype=torch.float64)) == 0
    assert rc.lsb_exp(torch.tensor([0.375, 4.0], dtype=torch.float64)) == -3
    assert rc.lsb_exp(torch.tensor([48.0, 16.0], dtype=torch.float64)) == 4
    assert rc.lsb_exp(torch.zeros(3, dtype=torch.float64)) == 0
