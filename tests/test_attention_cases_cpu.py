"""The case table of the attention tests (attention_cases.py), checked without a GPU and without the library: the table reaches every instantiation,
every tile schedule the build instantiates and every run-time branch, each named here, on both V^T load paths; the selection cases' score gaps and
integer ranges meet their preconditions; a plain float32 attention lies within the arithmetic bound; the NaN slack is where the layouts say."""
import os

import torch

import attention_cases as AC
from jatts_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, F32, F32S, F32E = AC.F16, AC.F32, AC.F32S, AC.F32E

# (arithmetic, d_k, KBT, REL, NW, schedule), written out from launch_attn and relattn_kernel's constexpr block: four arithmetics x six d_k ...
INSTANTIATIONS = (
    [(F16, dk, 64, True, 4, "prefetch") for dk in (32, 64, 96, 128, 192)] + [(F16, 256, 64, True, 4, "none")]       # f16 d_k 256: load and store back to back
    + [(F32, dk, 64, True, 4, "prefetch") for dk in (32, 64, 96)] + [(F32, dk, 32, True, 4, "dma") for dk in (128, 192, 256)]
    + [(F32, 256, 32, False, 4, "dma")]                                                                               # ... + the bias-free one (Matcha's)
    + [(F32S, dk, 64, True, 4, "prefetch") for dk in (32, 64, 96)] + [(F32S, dk, 32, True, 4, "prefetch") for dk in (128, 192)]
    + [(F32S, 256, 32, True, 8, "prefetch")]                                                                          # the 512-thread form IS split d_k 256
    + [(F32E, dk, 64, True, 4, "prefetch") for dk in (32, 64, 96)] + [(F32E, dk, 32, True, 4, "prefetch") for dk in (128, 192, 256)])


def test_constants_match_the_package():
    assert (AC.F32, AC.F16, AC.F32S, AC.F32E) == (_abi.F32, _abi.F16, _abi.F32S, _abi.F32E)
    assert {n for n, _ in _abi.RelAttnDesc._fields_} >= {"ldo", "vt_col0", "kv_len", "rel_mode", "rel_center"}


def test_restated_dispatch_gives_the_instantiations_written_out():
    """24 + the REL = false one = 25 distinct instantiations (the issue counts the NW = 8 form a second time: 26).  With the shipped JATTS_ATTN_DMA = 2
    every kernel that would take the register half-tile pipeline takes LDS-direct loads on the same schedule, so "half" is instantiated nowhere."""
    assert sorted(INSTANTIATIONS) == AC.ALL_INSTANTIATIONS and len(AC.ALL_INSTANTIATIONS) == 25
    assert {i[5] for i in AC.ALL_INSTANTIATIONS} == {"prefetch", "dma", "none"}
    old = AC.ATTN_DMA
    try:      # the logic itself does know the half pipeline: with DMA off the f32 d_k 256 kernels take it
        AC.ATTN_DMA = 0
        assert AC.instantiation(F32, 256, True, True)[5] == "half" and AC.instantiation(F32, 128, True, True)[5] == "prefetch"
    finally:
        AC.ATTN_DMA = old


def _facts(c):
    return [AC.seq_facts(c, b) for b in range(len(c.lens))]


def test_the_table_reaches_every_instantiation_and_branch():
    sel = {k: set() for k in AC.ALL_INSTANTIATIONS}
    ari = {k: set() for k in AC.ALL_INSTANTIATIONS}
    for c in AC.CASES:
        br = AC.branch(c)
        for f in _facts(c):
            if f["T"]:
                (ari if c.kind == "arith" else sel)[br].add((c.bias, f["vt_vec"]))
    for inst in AC.ALL_INSTANTIATIONS:
        forms = ["none"] if not inst[3] else AC.BIAS if (inst[0], inst[1]) != (F32, 256) else AC.BIAS[1:]
        want = {(b, v) for b in forms for v in (False, True)}
        assert ari[inst] >= want, (inst, sorted(want - ari[inst]))      # arithmetic: the bias forms x both V^T paths (8; f32 d_k 256: 2 + 6)
        assert sel[inst] >= want, (inst, sorted(want - sel[inst]))      # selection likewise
    # run-time branches, per instantiation family (arithmetic x tile size x schedule), named one by one
    fams = {}
    for c in AC.CASES:
        a, dk, kbt, rel, nw, sched = AC.branch(c)
        fam = fams.setdefault((a, kbt, nw, sched), set())
        for b, f in enumerate(_facts(c)):
            if not f["T"]:
                fam.add("empty-sequence")
                continue
            if c.kv is not None and c.kv[b] < 1:
                fam.add("kv-clamped-up")
            if c.kv is not None and c.kv[b] > f["T"]:
                fam.add("kv-clamped-down")
            fam.add("vt-vec" if f["vt_vec"] else "vt-elem")
            fam.add("tiles-1" if f["tiles"] == 1 else "tiles-many")
            fam.add("last-tile-partial" if f["last_partial"] else "last-tile-full")
            fam.add("wg-1" if f["wgs"] == 1 else "wg-many")
            fam.add("queries-clamped" if f["clamped_queries"] else "queries-full")
            fam.add("tk-" + f["tk_vs_tn"])
            if f["tk_vs_tn"] == "lt":
                fam.add("tk-edge-" + f["tk_vs_edge"])
            fam.update(f["gather"])
    need = {"vt-vec", "vt-elem", "tiles-1", "tiles-many", "last-tile-partial", "last-tile-full", "wg-1", "wg-many", "queries-clamped", "queries-full",
            "tk-eq", "tk-lt", "tk-edge-at", "tk-edge-after", "tk-edge-before", "tk-edge-inside", "kv-clamped-up", "kv-clamped-down", *AC.GATHER}
    assert len(fams) == 9      # f16 64 prefetch | none; f32 64 prefetch, 32 dma; split 64, 32, 32 NW 8; emul 64, 32
    for fam, got in fams.items():
        assert got >= need, (fam, sorted(need - got))
    assert any("empty-sequence" in got for got in fams.values())
    # the table's winners come through every gather branch, in every arithmetic
    for a in AC.ARITHS:
        won = set().union(*(AC.winner_gather(c) for c in AC.CASES if c.kind == "rel" and c.arith == a))
        assert won == set(AC.GATHER), (a, won)
    # the 1-D grid's decode: fewer than 8 workgroups, 8 k + 1, 8 k + 7 and whole multiples of 8; the NW = 8 kernel with two query workgroups
    totals = {AC.grid_total(c) for c in AC.CASES if c.group == "grid"}
    assert {1, 9, 39, 16} <= totals and any(t % 8 == 1 and t > 8 for t in totals) and any(t % 8 == 0 and t >= 16 for t in totals)
    assert any(AC.branch(c)[4] == 8 and f["wgs"] == 2 for c in AC.CASES for f in _facts(c))
    # the NW = 8 and the REL = false kernels under kv_len, the models' fused layout and H = 1, 2, 3 in every arithmetic
    assert any(AC.branch(c)[4] == 8 and c.kv for c in AC.CASES) and any(not AC.branch(c)[3] and c.kv for c in AC.CASES)
    for a in AC.ARITHS:
        assert {c.H for c in AC.CASES if c.arith == a} >= {1, 2, 3}
        assert {c.kind for c in AC.CASES if c.arith == a and c.qk == "fused"} >= {"qk", "arith"}
        assert any(c.ldo_extra for c in AC.CASES if c.arith == a) and any(0 in c.lens[1:-1] for c in AC.CASES if c.arith == a)
        assert {c.bias for c in AC.CASES if c.arith == a and c.group == "alone"} == {"none", "legacy", "new"}


def test_sizes_stay_inside_the_issues_set():
    for c in AC.CASES:
        assert c.H <= 3 and len(c.lens) <= 13, c.id
        assert set(c.lens) <= set(AC.LENGTHS) | {0, 3}, c.id
        assert c.cap > c.Tm and c.dk in AC.DKS
    assert AC.LENGTHS == [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130]
    for a, dk in {(c.arith, c.dk) for c in AC.CASES if c.group == "mask"}:
        kbt = AC.instantiation(a, dk, False, False)[2]
        assert AC.kv_values(kbt, 130) == [1, kbt, kbt - 1, kbt + 1, 130, 0, 135]


def test_every_case_is_in_bounds_by_construction():
    """What the kernel addresses, from its own index expressions, against what tensors() allocates."""
    for c in AC.CASES:
        off, ldvt, col0 = c.vt_geometry()
        ldq, qc0, ldk, kc0 = c.qk_layout()
        assert ldq % 8 == 0 and ldk % 8 == 0 and qc0 % 8 == 0 and kc0 % 8 == 0 and qc0 + c.A <= ldq and kc0 + c.A <= ldk, c.id
        end = 0
        for b, T in enumerate(c.lens):
            c0 = c.row0(b) if col0 is None else col0[b]
            assert c0 >= end and c0 + T <= ldvt, c.id                                  # sequences do not overlap in V^T
            end = c0 + T
            if c.vt_vec(b):
                assert c0 + AC.round_up(T, 8) <= ldvt, c.id                            # the 16-byte chunks of the last column block stay inside the row
            if c.bias == "legacy":
                assert T <= c.n_pos                                                    # g_q[Tn - 1 - qi + j], g_q1[j - qi - 2]
            if c.bias == "new":
                assert c.center - (T - 1) >= 0 and c.center + T - 1 < c.n_pos          # g_q[center - qi + j]
            if c.kv is not None:
                assert 1 <= c.tk(b) <= T
        assert c.ldo >= c.A and c.n_pos <= c.ldg or not c.has_g


def test_selection_cases_meet_their_preconditions():
    for c in AC.CASES:
        if not c.exact:
            continue
        q, k, v, ku, g = c.data
        assert torch.equal(v, v.round()) and float(v.abs().max()) <= 1023 and float(v.abs().min()) >= 1, c.id
        assert torch.equal(v.half().float(), v) and torch.equal(v.bfloat16().float() + (v - v.bfloat16().float()).bfloat16().float(), v)
        rows = c.exact_rows()
        r = c.ref
        assert float(r["gap"][rows].min()) >= 400.0, (c.id, float(r["gap"][rows].min()))      # __expf(-400) = 0: the softmax is one-hot in f32
        assert torch.equal(r["out"][rows].float(), c.expected()[rows]), c.id                    # and float64 agrees on the winner
        if c.kind == "qk":
            assert set(q.unique().tolist()) <= {-1.0, 1.0} and set(k.unique().tolist()) <= {-1.0, 1.0}
            o = 0
            for b, T in enumerate(c.lens):      # q_i . k_j = d_k at the winner, <= 3/4 d_k at every other key (the mask's duplicates aside)
                if T == 0:
                    continue
                dots = torch.einsum("ihc,jhc->hij", q[o:o + T], k[o:o + T])[:, :, :c.tk(b)]
                top = dots.topk(min(2, c.tk(b)), -1).values
                assert bool((top[..., 0] == c.dk).all()) and (c.tk(b) == 1 or float(top[..., -1].max()) <= 0.75 * c.dk), c.id
                if c.kv is not None and c.tk(b) < T:      # the winner's code stands right behind the mask too
                    assert torch.equal(k[o + c.tk(b)], k[o]) and bool((c.pi(b, 0) == 0).any())
                o += T
        elif c.kind == "qk11":
            for t in (q, k):
                assert set(t.abs().unique().tolist()) == {256.0, 257.0} and bool((t.bfloat16().float().abs() == 256).all()), c.id      # b0 = +-256, b1 = +-z
            o = 0
            for b, T in enumerate(c.lens):
                dots = torch.einsum("ihc,jhc->hij", q[o:o + T].double(), k[o:o + T].double())
                first = torch.einsum("ihc,jhc->hij", q[o:o + T].bfloat16().double(), k[o:o + T].bfloat16().double())
                base = (65536.0 + 256.0) * c.dk
                assert set(dots.unique().tolist()) == {base + c.dk / 4, base + c.dk / 2} and float(dots.max()) <= 2 ** 24 * (1 + 2.0 ** -7), c.id
                assert first.unique().numel() == 1      # without the second terms every key ties
                o += T
        elif c.kind in ("rel", "relneg"):
            assert not q.any() and not k.any() and ku is None
            fin = g[~g.isnan()]
            assert set(fin.unique().tolist()) == ({-1.0} if c.kind == "relneg" else {0.0, 1.0})
            if c.kind == "rel":
                assert int(fin.sum()) == c.R * c.H                                               # one 1 per (query, head)
        else:
            assert not q.any() and not k.any() and set(ku.unique().tolist()) == {-1.0, 0.0}
        # every head and every sequence has its own values
        assert c.H == 1 or not torch.equal(v[:, 0], v[:, 1])
        AC.release(c)


def test_rel_tables_are_poisoned_outside_what_the_shift_addresses():
    for c in AC.CASES:
        if not c.has_g or c.group not in ("sel", "wrap", "empty"):
            continue
        g, o = c.data[4], 0
        for T in c.lens:
            if T:
                probe = g[o:o + T].permute(1, 0, 2)
                assert bool(probe.isnan().any()) or T == c.Tm_table == c.n_pos
                assert not bool(c.shift(probe, T).isnan().any()), c.id      # no NaN slot is ever mapped to a score
            o += T
        AC.release(c)


def test_arithmetic_cases_exercise_what_they_claim_and_f32_fits_the_bound():
    worst = {}
    for c in AC.CASES:
        if c.exact:
            continue
        q, k, v, ku, g = c.data
        for t in (q, k, v):
            assert float(t.abs().min()) >= 2.0 ** -6 and float(t.abs().max()) <= 2.0 ** 7, c.id
        if c.arith == F16:
            assert all(t is None or torch.equal(t.half().float().nan_to_num(), t.nan_to_num()) for t in (q, k, v, g))
        else:      # full significands: the last of the 24 bits is in use
            assert float((torch.frexp(q)[0] * 2 ** 24 % 2).sum()) > 0.3 * q.numel()
        r = c.ref
        assert 1.0 <= float(r["kappa"].max()) <= 12.0, (c.id, float(r["kappa"].max()))      # |score| <~ 8 (+ the u . k and table terms)
        kbt = AC.branch(c)[2]
        o, rises, first, scales = 0, 0, 0, set()
        for b, T in enumerate(c.lens):
            tk = c.tk(b)
            if tk > kbt:
                # exponents of the tile maxima of K and V: they change from tile to tile, up and down
                ke = [int(torch.frexp(k[o + j:o + min(j + kbt, T)].abs().max())[1]) for j in range(0, tk, kbt)]
                ve = [int(torch.frexp(v[o + j:o + min(j + kbt, T)].abs().max())[1]) for j in range(0, tk, kbt)]
                scales.update(b_ - a_ for a_, b_ in zip(ve, ve[1:]))
                if kbt == 32 and tk > 64:
                    assert len(set(ke)) > 1, c.id
                # the running maximum: where is each row's best key
                qs, ks = q[o:o + T].double().transpose(0, 1), k[o:o + tk].double().transpose(0, 1)
                s = qs @ ks.transpose(1, 2)
                if ku is not None:
                    s = s + ku[o:o + tk].double().t().unsqueeze(1)
                best = s.argmax(-1) // kbt
                rises += int((best == (tk - 1) // kbt).sum())
                first += int((best == 0).sum())
            o += T
        if max(c.tk(b) for b in range(len(c.lens))) >= 130:
            assert rises > 0 and first > 0 and any(d > 0 for d in scales) and any(d < 0 for d in scales), (c.id, rises, first, scales)
        # a plain float32 attention of the same operands lies within the f32 bound (and, a fortiori, within the wider ones): the bound is not tighter
        # than an honest evaluation in the format
        r32 = c.attention(torch.float32)
        err = (r32["out"].double() - r["out"]).abs()
        ratio = float((err / c.bound(F32)).max())
        assert ratio <= 1.0, (c.id, ratio)
        assert float(err.max()) > 0
        for a in AC.ARITHS:
            assert bool((c.bound(a) >= c.bound(F32)).all())
        worst[c.arith] = max(worst.get(c.arith, 0.0), ratio)
        AC.release(c)
    assert set(worst) == set(AC.ARITHS)


def test_nan_slack_is_where_the_layouts_say():
    seen = set()
    for c in AC.CASES:
        if c.group not in ("layout", "losevec", "empty", "heads") and not (c.group == "arith" and c.dk == 32):
            continue
        t = AC.tensors(c)
        for name, mask in t["covered"].items():
            if name == "out":
                assert bool(t["out"].isnan().all()) and int(mask.sum()) == c.R * c.A
                continue
            buf = t[name]
            assert buf.data_ptr() % 64 == 0 and torch.equal(~buf.isnan(), mask), (c.id, name)
            seen.add((c.qk, name))
        assert t["vt"].data_ptr() % 32 == c.vt_props(0)["ptr"]
        assert bool(t["vt_buf"][-16:].isnan().all())
        AC.release(c)
    assert {("fused", "qk_buf"), ("wide", "q"), ("wide", "k"), ("sep", "vt_buf")} <= seen


def test_lose_vec_cases_differ_in_exactly_one_property():
    n = 0
    for c in AC.CASES:
        if c.group != "losevec" or c.name == "packed-aligned":
            continue
        for b in range(len(c.lens)):
            broken = [k for k, v in c.vt_props(b).items() if v]
            assert broken == ([] if c.name == "aligned" else [c.name]) and c.vt_vec(b) == (c.name == "aligned"), (c.id, broken)
        n += c.name != "aligned"
    assert n == 3 * 4 * 2      # three ways x four arithmetics x two d_k (64-key prefetch tiles; 32-key tiles: dma, split, emulated)
    for c in AC.CASES:
        if c.name == "packed-aligned":
            assert all(c.vt_vec(b) for b in range(2)) and c.vt_geometry()[2] is None


def test_alone_cases_keep_the_operands():
    c = AC.BY_ID["alone/f32-dk64/legacy"]
    whole, o = c.data, 0
    for b, T in enumerate(c.lens):
        one = c.alone(b)
        assert one.scale == c.scale and (one.n_pos, one.center, one.ldg) == (c.n_pos, c.center, c.ldg)
        for x, y in zip(one.data, whole):
            assert (x is None) == (y is None) and (x is None or torch.equal(x.nan_to_num(), y[o:o + T].nan_to_num()))
        o += T


def test_write_case_table():
    """profiles/attention_cases.txt: case -> layouts -> branch -> criterion."""
    lines = ["# case  H lens [kv]  bias/u.k  Q,K (ldq q0 ldk k0) | V^T (off ld col0) | ldo  ->  arith DK KBT REL NW schedule | per sequence: "
             "vec tiles(partial) wgs(clamped) gather  ->  criterion"]
    for c in AC.CASES:
        a, dk, kbt, rel, nw, sched = AC.branch(c)
        off, ldvt, col0 = c.vt_geometry()
        per = []
        for f in _facts(c):
            if not f["T"]:
                per.append("empty")
                continue
            gather = ",".join(s.split("-")[1] for s in AC.GATHER if s in f["gather"])
            per.append(f"{'v' if f['vt_vec'] else 'e'}{f['tiles']}{'p' if f['last_partial'] else ''}/{f['wgs']}{'c' if f['clamped_queries'] else ''}"
                       + (f"/{gather}" if gather else ""))
        if len(set(per)) == 1:
            per = [f"{len(per)}x {per[0]}"] if len(per) > 1 else per
        lines.append(f"{c.id}  H{c.H} {c.lens}{' kv' + str(c.kv) if c.kv else ''}  {c.bias}{'+ku' if c.ku_on and c.bias != 'ku' else ''}  "
                     f"{c.qk}{c.qk_layout()} | {c.vt}({off} {ldvt} {'row0' if col0 is None else 'col0'}) | {c.ldo}  ->  "
                     f"{AC.ANAME[a]} {dk} {kbt} {int(rel)} {nw} {sched} | {' '.join(per)}  ->  {c.criterion()}")
    path = os.path.join(ROOT, "profiles", "attention_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert os.path.getsize(path) < 1 << 20
