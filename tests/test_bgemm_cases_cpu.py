"""The case table of the batched-GEMM tests (bgemm_cases.py), checked without a GPU and without the library: every case reaches the branch
it names and the table reaches every instantiation; the integer cases are exact by construction; the arithmetic cases' own f32 evaluation
lies within their bound; the NaN slack is where the layouts say; the lose-the-16-byte-path cases each break one property."""
import os

import torch

import bgemm_cases as BC
from jatts_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENT = [(False, False), (False, True), (True, False), (True, True)]      # (AK, BKC): K contiguous in A / in B

# (WNF, BK, MF, vec), written out from jatts_bgemm's dispatch: six launch classes ...
EXACT = [(3, 16, 1, False), (2, 16, 2, False), (3, 16, 1, True), (3, 16, 2, True), (1, 32, 2, True), (2, 32, 2, True)]
# ... and from bgemm_emul_launch's: four tiles x 16-byte / element loads
EMUL = [(1, 32, 2, True), (1, 32, 2, False), (2, 32, 2, True), (2, 32, 2, False), (3, 32, 2, True), (3, 32, 2, False), (3, 32, 1, True),
        (3, 32, 1, False)]


def test_constants_match_the_package():
    assert BC.F32E == _abi.F32E


def test_every_case_reaches_the_branch_it_names():
    for c in BC.CASES:
        kern, wnf, bk, mf, vec, ak, bkc = BC.branch(c)
        assert kern == c.kernel and (ak, bkc) == (not c.ta, c.tb), c.id
        if c.expect is not None:
            assert (wnf, bk, mf, vec) == c.expect, (c.id, (wnf, bk, mf, vec), c.expect)
        assert vec == BC.is_vec(c)
    # the only forced tiles: the one the dispatcher cannot reach, and the one-bit-pattern group
    assert {c.group for c in BC.CASES if c.tile} == {"inst", "bits"}
    assert {BC.branch(c)[1:5] for c in BC.CASES if c.tile and c.group == "inst"} == {(3, 32, 2, False)}


def test_the_table_reaches_every_instantiation():
    full = sorted([("exact",) + cls + o for cls in EXACT for o in ORIENT] + [("emul",) + cls + o for cls in EMUL for o in ORIENT])
    assert len(full) == 24 + 32 and full == BC.ALL_BRANCHES
    for integer in (True, False):      # by integer cases alone, and by arithmetic cases alone
        reached = sorted({BC.branch(c) for c in BC.CASES if c.exact == integer})
        assert reached == full, (integer, sorted(set(full) - set(reached)))
    # the 128 x 192 tile by count, on both sides of 1024 workgroups
    by_count = {c.name: BC.branch(c)[3] for c in BC.CASES if c.group == "count" and c.kernel == "exact"}
    assert by_count == {"1024": 2, "1023": 1}
    # K edges at both chunk depths of the exact kernel and the emulated kernel's one
    assert {BC.branch(c)[:3:2] for c in BC.CASES if c.group == "kedge"} == {("exact", 16), ("exact", 32), ("emul", 32)}


def test_integer_cases_are_exact_by_construction():
    for c in BC.CASES:
        if not c.exact:
            continue
        a, b = c.data
        assert torch.equal(a, a.round()) and torch.equal(b, b.round()), c.id
        assert c.magnitude() < BC.F24, (c.id, c.magnitude())                     # sum |a| |b| (+ the start pattern): no partial sum in any order leaves the integers of f32
        assert torch.equal(c.expected(), (c.expected() * 2).round() / 2) and torch.equal(c.expected().float().double(), c.expected()), c.id
        if c.gen == "odd16":
            assert c.k <= 64 and float(a.abs().max()) < 2 ** 16 and float(a.abs().min()) > 256 and bool((a.long() % 2 == 1).all())
            assert bool((a.bfloat16().float() != a).all()), c.id                 # a second bf16 term everywhere
            assert set(b.unique().tolist()) <= {-2.0, -1.0, 1.0, 2.0}
        else:
            assert float(a.abs().max()) <= 4 and float(b.abs().max()) <= 4
        for t in (a, b):                                                         # every matrix of a batch has its own data
            mats = t.reshape(-1, *t.shape[2:])
            assert mats.shape[0] == 1 or not bool((mats[1:] == mats[:-1]).flatten(1).all(1).any()), c.id
        BC.release(c)


def test_arithmetic_reference_lies_within_its_own_bound():
    seen = set()
    for c in BC.CASES:
        if c.exact:
            continue
        a, b = c.data
        assert c.k in (1, 8, 33, 70) and float(a.min()) >= 2.0 ** -6 and float(a.max()) <= 2.0 ** 7 and float(b.min()) > 0
        assert torch.equal(c.ref, c.absref)                                      # all positive: nothing cancels
        err, bound = (c.ref32.double() - c.ref).abs(), c.bound()
        assert bool((err <= bound).all()), (c.id, float((err / bound).max()))
        assert float(err.max()) > 0 or c.k == 1                                  # (the f32 evaluation does round: the check is not vacuous)
        seen.add((c.kernel, c.k))
        BC.release(c)
    assert seen >= {(kern, k) for kern in ("exact", "emul") for k in (1, 8, 33)}
    assert BC.bound_factor("exact", 8) == 10 and BC.bound_factor("emul", 8) == 1.05 * 8 + 3


def test_nan_slack_is_where_the_layouts_say():
    nan_after_operand = 0
    for c in BC.CASES:
        a, b = c.data
        for layout, shape, vals in ((c.la, c.a_shape(), a), (c.lb, c.b_shape(), b), (c.lc, c.c_shape(), None)):
            if c.group == "count" and vals is None:
                continue                                                         # (35 MB, contiguous)
            idx, size = BC.covered(layout, shape)
            assert idx.unique().numel() == idx.numel(), (c.id, layout)           # no two elements share an address
            if vals is None:
                continue
            buf, view = BC.place(layout, shape, vals)
            assert buf.numel() == size and buf.data_ptr() % 16 == 0
            assert view.data_ptr() % 16 == 4 * (layout.off % 4) and view.stride() == (layout.so, layout.si, layout.ld, 1)
            mask = torch.ones(size, dtype=torch.bool)
            mask[idx] = False
            assert torch.equal(buf.isnan(), mask) and torch.equal(view, vals), (c.id, layout)
            if c.group == "straddle":      # NaN right behind a row whose last 16-byte piece is partial
                rows, cols = shape[2:]
                assert cols % 4 != 0 and layout.ld % 4 == 0 and bool(buf[layout.off + cols:layout.off + layout.ld].isnan().all())
                nan_after_operand += int(layout.si > rows * layout.ld)
        BC.release(c)
    assert nan_after_operand > 0                                                 # and between matrices in the gap4 layouts


def test_lose_vec_cases_differ_in_exactly_one_property():
    n = 0
    for c in BC.CASES:
        if c.group != "losevec":
            continue
        props = {f"{op}.{k}": v for op, layout in (("a", c.la), ("b", c.lb)) for k, v in layout.vec_props().items()}
        assert sorted(props) == sorted(BC.LOSE_VEC)
        broken = [k for k, v in props.items() if v]
        if c.name == "aligned":
            assert broken == [] and BC.is_vec(c)
        else:
            assert broken == [c.name] and not BC.is_vec(c), (c.id, broken)
            assert props[c.name] == (1 if c.name.endswith("ptr") else 2)
            n += 1
    assert n == 8 * 4 * 2      # eight ways x four forms x two kernels


def test_case_lists_of_the_issue():
    by = lambda g, k="exact": [c for c in BC.CASES if c.group == g and c.kernel == k]  # noqa: E731
    assert BC.M_EDGES == [1, 63, 64, 65, 127, 128, 129] and BC.N_EDGES == [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]
    assert {c.m for c in by("medge")} == set(BC.M_EDGES) and {c.n for c in by("nedge", "emul")} == set(BC.N_EDGES)
    assert BC.k_edges(16) == [1, 15, 16, 17, 32, 33, 53] and BC.k_edges(32) == [1, 31, 32, 33, 64, 65, 101]
    assert {(c.O, c.I) for c in by("batch")} == {(1, 1), (7, 1), (1, 8), (3, 3), (17, 1), (5, 7), (2, 48)}
    assert all((c.m, c.n) == (130, 70) and c.k in (9, 27) for c in by("batch") + by("batch", "emul"))
    assert {(c.alpha, c.acc) for c in by("store")} >= {(0.5, 1), (-2.0, 1), (0.5, 2)}
    (big,) = [c for c in by("count") if c.name == "1024" and (c.ta, c.tb) == (False, True)]
    assert (big.O, big.I, big.m, big.n, big.k) == (128, 8, 65, 132, 20)


def test_write_case_table():
    """profiles/bgemm_cases.txt: case -> branch -> criterion."""
    lines = ["# case  (O, I, m, n, k)  A layout | B layout | C layout  ->  kernel WNF BK MF vec AK BKC  ->  criterion"]
    for c in BC.CASES:
        kern, wnf, bk, mf, vec, ak, bkc = BC.branch(c)
        extra = "".join([f" alpha={c.alpha}" if c.alpha != 1 else "", f" accumulate x{c.acc}" if c.acc else "", " forced" if c.tile else ""])
        lines.append(f"{c.id}  {(c.O, c.I, c.m, c.n, c.k)}  {c.la} | {c.lb} | {c.lc}  ->  {kern} {wnf} {bk} {mf} {'vec' if vec else 'elem'} "
                     f"{int(ak)} {int(bkc)}  ->  {c.criterion()}{extra}")
    path = os.path.join(ROOT, "profiles", "bgemm_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert os.path.getsize(path) < 1 << 20
