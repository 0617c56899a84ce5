"""CPU side of the conv1d store suite (tests/conv_store_cases.py, tests/test_conv_store_gpu.py): the preconditions of exactness proven from the
generated data, the epilogue-selection model held to the text of the sources, the proof that the table reaches every store path of every kernel and
flips every predicate alone, and the sensitivity of the comparison to six deliberately wrong store geometries.  `pytest -s` prints the
kernel -> case -> path table of profiles/r35_notes.md."""
import collections

import pytest
import torch

import conv_store_cases as cs
import test_conv_geometry_gpu as geo          # (_variants: the kernels and forced tiles of an arithmetic; nothing there touches a GPU at import)


def kernels(arith):
    """[(label, w_layout, variant, y16)]: _variants(arith, every_tile=True), plus the F32 register-streamed ring-4 kernel (variant 4)."""
    out = [(label, layout, kw.get("variant", 0), label == "y16") for label, layout, kw in geo._variants(arith, every_tile=True)]
    return out + [("v4", 0, 4, False)] if arith == "F32" else out


def applies(case, arith, y16):
    """Does the case LAUNCH in this kernel?  An f16 y cannot alias the f32 residual (hip.conv1d refuses the dtype); the split / emulated kernels refuse halos
    beyond 32 rows (their PreparedWeight forms run the F32 kernel instead)."""
    if y16 and case.r and case.r[0] in ("inplace", "vits"):
        return False
    return not (cs.wide_halo(case) and arith in ("F32S", "F32E", "F32E6"))


@pytest.mark.parametrize("name", [c.name for c in cs.CASES])
def test_preconditions_of_exactness(name):
    case, d = cs.BY_NAME[name], cs.data(name)
    k, dil, pad = case.geom
    assert 0 <= pad <= (k - 1) * dil and case.alpha in (1.0, 0.5, 2.0)
    if case.reflect:
        assert min(case.lens) >= cs.halo_of(case) + 1
    # every partial sum of z, in any order, is an integer below 2**24
    bound = float(d.x.abs().max()) * float(d.w.abs().sum((1, 2)).max()) + float(d.b.abs().max())
    assert bound < cs.F24 and float(d.x.abs().max()) <= 8 and float(d.w.abs().max()) <= 4
    assert len(d.xs) == case.n_in and torch.equal(sum(d.xs), d.x)
    for t in (d.x, d.w, d.b, *d.xs):
        assert torch.equal(t, t.round()) and torch.equal(t.half().float(), t), "operands are integers, exact in f16"
    assert torch.equal(d.z, d.z.round()) and float(d.z.abs().max()) <= bound
    if d.rbuf is not None:
        assert torch.equal(d.rbuf, d.rbuf.round()) and float(d.rbuf.abs().max()) <= 8
    if case.act in cs.NONLINEAR:
        # the saturating range and the curved one are both in the data
        assert int((d.z.abs() > 100).sum()) > 100 and int((d.z.abs() <= 2).sum()) > 10, (float(d.z.abs().max()), int((d.z.abs() <= 2).sum()))
        err32, tol, _, _ = cs.bound(name)
        assert cs.T_K <= tol < 1e-4, (err32, tol)            # the reference side's own f32 error stays in the range of T_k
        return
    val = cs.value(case)
    za = torch.relu(d.z) * case.alpha if case.act == "relu" else d.z * case.alpha
    # act(z) * alpha is exact (a power of two times an integer), and adding the residual is exact too: FMA or not, the same number
    assert torch.equal(za.float().double(), za) and torch.equal(val.float().double(), val) and torch.equal(2 * val, (2 * val).round())
    # every f16-stored result is an f16 number: integers below 2048, half-integers below 1024
    whole = torch.equal(val, val.round())
    assert float(val.abs().max()) < (cs.F16_EXACT if whole else cs.F16_EXACT // 2), (name, float(val.abs().max()), whole)
    assert torch.equal(val.half().double(), val)
    print(f"{name}: max |z| = {float(d.z.abs().max()):.0f}, max |y| = {float(val.abs().max()):g}, bound on partial sums {bound:.0f}")


@pytest.mark.parametrize("fname", sorted(cs.SOURCE_PREDICATES))
def test_model_quotes_the_sources(fname):
    """The selection rules the model evaluates are, statement for statement, the ones in the source file -- no rule more, none less, none reworded.  A change
    to a selection rule fails here until the model and the table have been revisited."""
    src = cs.source_predicates(fname)
    model = {cs.normalise(v) for v in cs.SOURCE_PREDICATES[fname].values()}
    assert src == model, f"{fname}: only in the source: {sorted(src - model)}; only in the model: {sorted(model - src)}"


def _model_paths(arith, layout, variant, y16):
    out = set()
    for L in cs.model_launches():
        if bool(L.y_is_f32) == (not y16):
            out.add(cs.store_path(arith, layout, variant, L))
    return out


def _table():
    """{(arith, label): {axis: {path: [case names]}}} over every launch of the GPU module."""
    tab = collections.OrderedDict()
    for arith in cs.ARITHS:
        for label, layout, variant, y16 in kernels(arith):
            row = tab.setdefault((arith, label), collections.OrderedDict((a, collections.OrderedDict()) for a in cs.AXES))
            for case in cs.CASES:
                if applies(case, arith, y16):
                    row[case.axis].setdefault(cs.store_path(arith, layout, variant, cs.launch_of(case, arith, y16)), []).append(case.name)
    return tab


def test_table_reaches_every_store_path_of_every_kernel():
    tab, missing = _table(), []
    for arith in cs.ARITHS:
        for label, layout, variant, y16 in kernels(arith):
            row = tab[(arith, label)]
            reached = {p for axis in row.values() for p in axis}
            possible = _model_paths(arith, layout, variant, y16)
            print(f"\n{arith} {label or '-'}: {len(reached)} paths")
            for axis, paths in row.items():
                print(f"  {axis:14s} " + "; ".join(f"{p} [{' '.join(names)}]" for p, names in paths.items()))
            if reached != possible:
                missing.append(f"{arith} {label}: unreached {sorted(possible - reached)}; outside the model's grid {sorted(reached - possible)}")
    assert not missing, "\n".join(missing)


def test_no_instantiated_tile_misses_the_lds_limit():
    """The 160 / 159 KiB term of the f32_tile conditions holds for every tile the dispatchers instantiate (one input or several), so no launch can flip it: it is the
    one predicate term the table cannot (and need not) reach."""
    for arith in cs.ARITHS:
        for label, layout, variant, y16 in kernels(arith):
            for L in cs.model_launches():
                fam, BT, BN = cs.tile_of(arith, layout, variant, L)
                assert BT * (BN * 4 + 16) <= 159 * 1024, (arith, label, fam, BT, BN)


def test_every_predicate_is_flipped_alone():
    """For every predicate atom of the selection and every arithmetic: two table launches through one kernel differ in that atom and in nothing else (but what
    the atom drags along: COUPLED); across the kernels, at least one such pair changes the store path."""
    for arith in cs.ARITHS:
        for atom in cs.ATOMS:
            if atom in ("y_is_f32", "ldy % 8 == 0") and arith != "F16":      # (the f16 tile's two own terms: no predicate of the f32-storing kernels)
                continue
            flips, changed = 0, 0
            for label, layout, variant, y16 in kernels(arith):
                runs = [(c, cs.launch_of(c, arith, y16)) for c in cs.CASES if applies(c, arith, y16)]
                if atom == "y_is_f32":
                    runs += [(c, cs.launch_of(c, arith, not y16)) for c in cs.CASES if applies(c, arith, not y16)]
                vecs = [(c, L, cs.atoms_of(L)) for c, L in runs]
                for i, (ca, La, va) in enumerate(vecs):
                    for cb, Lb, vb in vecs[i + 1:]:
                        diff = {k for k in va if va[k] != vb[k]}
                        if atom in diff and None not in (va[atom], vb[atom]) and diff - {atom} <= cs.COUPLED.get(atom, set()):
                            flips += 1
                            changed += cs.store_path(arith, layout, variant, La) != cs.store_path(arith, layout, variant, Lb)
            print(f"{arith}: '{atom}' flipped alone by {flips} launch pairs, {changed} of them change the path")
            assert flips > 0 and changed > 0, f"{arith}: no table case flips '{atom}' alone" if not flips else f"{arith}: flipping '{atom}' never changes a path"


FAULTS = [("resid_col_minus4", "residual"), ("partial_quad_unwritten", "n_out"), ("seq_col0_ignored", "transposed"), ("len_mul_dropped", "transposed"),
          ("alpha_after_resid", "act_exact"), ("first_output_n_out_wide", "split")]


@pytest.mark.parametrize("fault,axis", FAULTS, ids=[f for f, _ in FAULTS])
def test_wrong_store_geometries_are_detected(fault, axis):
    """A deliberately wrong reference differs from the true one on at least one case of its axis, and the comparison the GPU tests use rejects the one when
    handed the other (as an f32 and as an f16 `kernel output`)."""
    found = []
    for case in cs.of_axis(axis):
        wrong, true = cs.expected(case.name, fault), cs.expected(case.name)
        if wrong is None or cs.same_buffers(wrong, true):
            continue
        found.append(case.name)
        for dt in (torch.float32, torch.float16):
            with pytest.raises(AssertionError, match="differ from the integer reference|outside the output window|inside the output window"):
                cs.check_buffer(wrong.want.to(dt), true.want, case.name)
                if wrong.want2 is not None:
                    cs.check_buffer(wrong.want2.to(dt), true.want2, case.name)
            cs.check_buffer(true.want.to(dt), true.want, case.name)
    print(f"{fault}: detected on {found}")
    assert found, f"{fault}: no case of axis {axis} tells the wrong reference from the true one"


def test_check_buffer_sees_canaries_and_holes():
    want = torch.full((4, 8), cs.NAN, dtype=torch.float64)
    want[:, 2:6] = 3.0
    good = want.float()
    cs.check_buffer(good, want, "good")
    for r, c, v, msg in ((1, 6, 3.0, "outside the output window"), (2, 3, cs.NAN, "inside the output window"), (0, 2, 3.5, "differ from the integer reference")):
        y = good.clone()
        y[r, c] = v
        with pytest.raises(AssertionError, match=msg):
            cs.check_buffer(y, want, "bad")
    allowed = torch.full((4, 8), 1e-3, dtype=torch.float64)
    assert cs.check_buffer(good + 5e-4, want, "near", allowed) == pytest.approx(0.5, rel=1e-3)
    with pytest.raises(AssertionError, match="elementwise bound"):
        cs.check_buffer(good + 2e-3, want, "far", allowed)
