"""The case tables of the alignment-learning kernel tests (alignment_cases.py), checked without a GPU: the mirrored tile constants are the kernels',
the tables reach every structural class they are there for, the exact MAS inputs are exact and full of ties, the fixture holds the real reference's
paths and the oracle reproduces them, a `>` tie rule is caught, and every refusal is a host-side argument check that returns before any HIP call."""
import ctypes as C
import os

import numpy as np
import torch

import alignment_cases as AC
from oracle.mas_oracle import monotonic_alignment_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_constants_are_the_kernels():
    for fname, consts in AC.CONSTANTS.items():
        found = AC.hip_constants(fname)
        for name, value in consts.items():
            assert found[name] == value, (fname, name, found.get(name), value)
    assert AC.MAS_LDS_MAX == 163808 and AC.align_lds(492) <= AC.LDS_BYTES < AC.align_lds(493)
    assert AC.AL_FB * 512 == 256 * AC.AL_PAIRS and 256 * AC.MAS_SLOTS == 1024


# ---------------------------------------------------------------- MAS
def test_mas_table_reaches_every_class():
    cls = [AC.mas_class(*s) for s in AC.MAS_SHAPES]
    assert {c["W"] for c in cls} == {1, 2, 4, 5, 8, 9, 16}
    assert {c["slots"] for c in cls} == {1, 2, 3, 4}
    assert {c["mel_mod8"] for c in cls} >= {0, 1, 2}
    assert {c["order"] for c in cls} == {"<", "==", ">"}
    assert {ti for _, ti in AC.MAS_SHAPES} >= {63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024}
    ring = [tm for tm, ti in AC.MAS_SHAPES if ti == 5]
    assert ring == [2, 8, 9, 10, 16, 17, 18] and {AC.ceil_div(t - 1, AC.MAS_PF) for t in ring} == {1, 2, 3}      # 8k, 8k + 1, 8k + 2 columns
    # the issue's shapes, but for the two the kernel's LDS cannot hold
    issue = [(1, 1), (2, 1), (1, 2), (8, 9), (9, 9), (10, 9), (17, 16), (64, 63), (64, 64), (64, 65), (66, 65), (300, 255), (300, 256), (300, 257),
             (600, 511), (600, 513), (1100, 1023), (1100, 1024)]
    assert set(issue) - set(AC.MAS_SHAPES) == set(AC.MAS_REFUSED)
    assert all(AC.mas_lds(*s) > AC.LDS_BYTES for s in AC.MAS_REFUSED) and {(1085, 1023), (1085, 1024)} <= set(AC.MAS_SHAPES)
    assert [AC.mas_lds(*s) for s in AC.MAS_LIMIT_SHAPES] == [163804, 163732]
    assert all(AC.mas_lds(tm + 1, ti) > AC.MAS_LDS_MAX for tm, ti in AC.MAS_LIMIT_SHAPES)
    # every launch's batch maxima fit
    launches = AC.mas_launches(AC.MAS_SHAPES)
    assert len(launches) == 3 and sum(launches, []) == AC.MAS_SHAPES
    for group in launches:
        assert AC.mas_lds(max(t for t, _ in group), max(i for _, i in group)) <= AC.MAS_LDS_MAX
        assert len(group) >= 2


def test_mas_exact_inputs_are_exact_and_tie():
    for kind in AC.MAS_EXACT:
        for tm, ti in AC.MAS_SHAPES:
            codes, lp = AC.mas_input(kind, tm, ti)
            assert codes.dtype == np.int8 and lp.dtype == np.float32 and lp.shape == (tm, ti)
            assert np.array_equal(lp * 2, np.round(lp * 2)) and float(np.abs(lp).max()) <= 7.5 and tm * 7.5 < 2 ** 24      # |any path sum| < 2^24 halves
            assert set(np.unique(codes).tolist()) <= set(range({"q4": 4, "half": 16, "const": 3}[kind]))
            path, ties, _ = AC.mas_solved(kind, tm, ti)
            assert np.array_equal(path, monotonic_alignment_search(lp)), (kind, tm, ti)          # the model's Q is the oracle's
            assert np.array_equal(path, monotonic_alignment_search(lp, literal=True)), (kind, tm, ti)
            # T_inp = 1 has no decision to take (the path is all zeros): a tie needs two tokens
            if kind != "const" and tm > ti >= 2:
                assert ties >= 1, (kind, tm, ti)
            if kind == "const" and tm > ti >= 2:
                # every finite comparison ties, so the path is the tie rule alone: `>=` steps down a token at every frame from the end while it can
                assert ties >= 1 and np.array_equal(path, np.maximum(0, np.arange(tm) - (tm - ti)))
    assert {v for s in AC.MAS_SHAPES for v in np.unique(AC.mas_input("half", *s)[0]).tolist()} == set(range(16))
    # shapes of the kind the tie rule decides dozens of frames in
    assert AC.mas_solved("q4", 300, 257)[1] >= 4


def test_a_strict_tie_rule_is_caught():
    """The CPU-side equivalent of `>=` -> `>` in mas_kernel: the same DP with the wrong comparison takes another path on every case with slack."""
    for kind in AC.MAS_EXACT:
        differing = 0
        for tm, ti in AC.MAS_SHAPES:
            if not tm > ti >= 2:
                continue
            good, _, wrong = AC.mas_solved(kind, tm, ti)
            assert not np.array_equal(good, wrong), (kind, tm, ti)
            differing += 1
        assert differing >= 10
    # ... while random float log-softmax inputs, the only kind the suite had, cannot tell the two apart
    good, _, wrong = AC.mas_solved("rand", 300, 257)
    assert np.array_equal(good, wrong)


def test_mas_fixture_is_the_reference_and_the_oracle_matches_it():
    path = os.path.join(ROOT, "tests", "golden", "mas_ties.npz")
    assert os.path.getsize(path) < 200 * 1000
    z = np.load(path)
    assert sorted(z.files) == sorted(["shapes"] + [k + s for k in AC.MAS_EXACT for s in ("_codes", "_paths")])
    assert all(z[k + "_codes"].dtype == np.int8 and z[k + "_paths"].dtype == np.int64 for k in AC.MAS_EXACT)
    fix = AC.mas_fixture()
    assert sorted(fix) == sorted((k, tm, ti) for k in AC.MAS_EXACT for tm, ti in AC.MAS_FIXTURE_SHAPES)
    assert (300, 257) in AC.MAS_FIXTURE_SHAPES and max(ti for _, ti in AC.MAS_FIXTURE_SHAPES) == 257
    for (kind, tm, ti), (codes, ref) in fix.items():
        assert np.array_equal(codes, AC.mas_input(kind, tm, ti)[0]), (kind, tm, ti)              # the generator still makes what the reference saw
        lp = AC.mas_decode(kind, codes)
        assert lp.dtype == np.float32 and np.array_equal(lp.astype(np.float64), -AC.MAS_SCALE[kind] * codes.astype(np.float64))
        assert np.array_equal(monotonic_alignment_search(lp), ref), (kind, tm, ti)
        assert ref[-1] == ti - 1 and (tm < ti or ref[0] == 0) and bool(np.all(np.diff(ref) >= 0)) and bool(np.all(np.diff(ref) <= 1))


def _ragged(lib, max_len, n_seq=1):
    from jatts_amd import _abi
    scratch = (C.c_float * 64)()
    p = C.addressof(scratch)
    return scratch, p, _abi.Ragged(p, n_seq, max_len, 1, 0, None)


def test_mas_refusals_come_before_any_launch(lib):
    """jatts_mas_viterbi's argument checks (host scratch pointers: no kernel ever sees them).  (4408, 256) prices 163 840 bytes: inside 160 KiB, but
    not inside what the kernel's own static LDS leaves -- it used to pass the check and fail at the launch."""
    keep, p, _ = _ragged(lib, 1)
    for tm, ti, ld in [(4408, 256, 256), (1086, 1024, 1024)] + [(tm, ti, 1024) for tm, ti in AC.MAS_REFUSED]:
        assert AC.mas_lds(tm, ti) > AC.MAS_LDS_MAX
        _, _, rg = _ragged(lib, tm)
        assert lib.jatts_mas_viterbi(C.byref(rg), p, p, ld, ti, p, p, p, None) == ERR_UNSUPPORTED, (tm, ti)
        assert b"160 KiB" in lib.jatts_last_error()
    assert AC.mas_lds(4408, 256) == AC.LDS_BYTES
    _, _, rg = _ragged(lib, 8)
    assert lib.jatts_mas_viterbi(C.byref(rg), p, p, 1032, 1025, p, p, p, None) == ERR_UNSUPPORTED and b"1..1024" in lib.jatts_last_error()
    assert lib.jatts_mas_viterbi(C.byref(rg), p, p, 63, 64, p, p, p, None) == ERR_UNSUPPORTED and b"<= ld" in lib.jatts_last_error()
    _, _, rg = _ragged(lib, 0)
    assert lib.jatts_mas_viterbi(C.byref(rg), p, p, 8, 5, p, p, p, None) == 0          # nothing to do: no launch either
    del keep


# ---------------------------------------------------------------- alignment log-probabilities
def test_align_tables_reach_every_class():
    assert {k: (c.flens, c.tlens, c.adim) for k, c in zip(AC.ALIGN_BATCHES, AC.ALIGN_FWD_CASES)} == \
        {"A": ([17, 0, 1, 16, 33], [33, 5, 1, 64, 65], 65), "B": ([15, 2], [492, 31], 63), "C": ([33], [130], 384), "D": ([16, 17], [32, 63], 1),
         "E": ([31], [63], 64), "F": ([32, 1], [64, 32], 129)}
    fwd = [c.classes() for c in AC.ALIGN_FWD_CASES]
    assert {c["chunks"] for c in fwd} == {1, 2, 3, 6}
    assert {c["chunk_tail"] for c in fwd} == {0, 1, 63}
    assert set().union(*(c["nf"] for c in fwd)) >= {1, 2, 15, 16}
    strides = set().union(*(c["lane_strides"] for c in fwd))
    assert 1 in strides and 2 in strides and max(strides) > 2                        # tokens <= 64, 65..128, > 128
    assert max(max(c.tlens) for c in AC.ALIGN_FWD_CASES) == 492 and max(c["lds"] for c in fwd) == AC.align_lds(492) <= AC.LDS_BYTES
    assert any(c["fill"] > 0 for c in fwd) and all(c.ld >= max(c.tlens) for c in AC.ALIGN_BWD_CASES)
    bwd = [c.classes() for c in AC.ALIGN_BWD_CASES]
    assert AC.ALIGN_BWD_CASES[:6] == AC.ALIGN_FWD_CASES
    assert set().union(*(c["token_tiles"] for c in bwd)) >= {1, 2, 3, 5, 16}
    assert set().union(*(c["token_tail"] for c in bwd)) >= {0, 1, 31}
    assert set().union(*(c["frame_chunk_tail"] for c in bwd)) >= {0, 1, 31}
    assert any(c["zero_frames"] for c in bwd)
    by = {c.name: c for c in AC.ALIGN_BWD_CASES}
    assert (by["train"].flens, by["train"].tlens, by["train"].ld) == ([40] * 3, [17, 5, 1], 17)
    for b, cols in by["masked"].masked.items():      # two interior valid columns
        assert len(cols) == 2 and all(0 < j < by["masked"].tlens[b] - 1 for j in cols)
    b, f, j = by["coincident"].coincident
    feats, text, _ = by["coincident"].data
    assert torch.equal(feats[f], text[j]) and b == 0
    for c in AC.ALIGN_BWD_CASES:                     # finite garbage at every padded dlog_p column
        dlp, o = c.data[2], 0
        for fl, tl in zip(c.flens, c.tlens):
            assert bool((dlp[o:o + fl, tl:].abs() >= 1e3).all()) and bool(torch.isfinite(dlp).all())
            o += fl


def test_align_references_are_finite_and_the_forward_bound_is_not_vacuous():
    for c in AC.ALIGN_BWD_CASES:
        (lp, dist, dF, dT), (lp32, _, dF32, dT32) = c.ref, c.ref32
        assert all(bool(torch.isfinite(t).all()) for t in (dF, dT, dF32, dT32)), c.name       # the coincident row included
        for b, cols in c.masked.items():
            assert cols and bool(torch.isinf(lp[b][:, cols]).all()) and not bool(dT[sum(c.tlens[:b]):][cols].any())
        for b, fl in enumerate(c.flens):
            if fl == 0:
                assert not bool(dT[sum(c.tlens[:b]):sum(c.tlens[:b + 1])].any())
    for c in AC.ALIGN_FWD_CASES:
        for b, fl in enumerate(c.flens):
            if fl == 0:
                continue
            bound = c.fwd_bound(b)
            # a dropped channel moves a distance by ~ dist / (2 adim) (0.04 at 384 channels), a dropped token the log-sum-exp by its probability
            assert 4 * AC.U <= float(bound.min()) and float(bound.max()) < 1e-3 and float(bound.max()) < 0.05 * float(c.ref[1][b].mean()) / (2 * c.adim)


def test_align_refusals_come_before_any_launch(lib):
    keep, p, rg = _ragged(lib, 16)
    for tl, ld, msg in ((493, 496, b"too long for LDS"), (513, 520, b"1..512"), (40, 39, b"<= ld")):
        assert lib.jatts_alignment_logp(C.byref(rg), p, tl, p, p, 8, p, ld, None) == ERR_UNSUPPORTED and msg in lib.jatts_last_error(), tl
        assert lib.jatts_alignment_logp_bwd(C.byref(rg), p, tl, p, p, 8, p, ld, p, ld, p, p, p, None) == ERR_UNSUPPORTED, tl
        assert msg in lib.jatts_last_error()
    assert lib.jatts_alignment_logp_bwd(C.byref(rg), p, 40, p, p, 8, p, 40, p, 39, p, p, p, None) == ERR_UNSUPPORTED      # ld_g too
    del keep


# ---------------------------------------------------------------- Gaussian upsampling
def test_gauss_table_reaches_every_class():
    assert {k: v for k, v in AC.GAUSS_BATCHES.items() if k != "H"} == {
        "A": ([1, 2, 3, 0], [5, 1, 0, 4], 3, 5, 1), "B": ([17, 16, 15], [31, 32, 33], 17, 33, 20), "C": ([63, 64, 65], [63, 64, 65], 65, 65, 33),
        "D": ([512, 500], [65, 10], 512, 65, 31), "E": ([33], [130], 33, 130, 129), "F": ([9, 4], [40, 64], 9, 64, 384), "G": ([8, 8], [32, 32], 8, 32, 128)}
    cls = [c.classes() for c in AC.GAUSS_CASES]
    union = lambda k: set().union(*(c[k] for c in cls))  # noqa: E731
    assert union("kv_parity") == {0, 1}
    assert union("k2_mod16") >= {0, 2, 4, 8}
    assert union("frame_tail") >= {0, 1, 63} and {c["store_tail"] for c in cls} >= {0, 1}
    assert {c["bwd_chunk_tail"] for c in cls} >= {0, 1}
    assert any(c["padded_tiles"] for c in cls) and any(c["partial_tiles"] for c in cls)
    cs = {c["C"] for c in cls}
    assert min(cs) < 32 and {32, 33, 128, 129} <= cs and any(c["wave_passes"] > 1 for c in cls) and 384 in cs
    assert any(c["kv0"] for c in cls) and any(c["kvo0"] for c in cls) and max(c["Tm"] for c in cls) == AC.GU_TMAX
    for c in AC.GAUSS_CASES:
        hs, ds, g = c.data
        assert torch.equal(ds, ds.round()) and float(ds.min()) >= 0
        for b, n in enumerate(c.kv):
            assert not bool(ds[b, n:].any()) and (n == 0 or float(ds[b, 0]) == 0.0 or (c.name, b) == ("F", 1))      # (F[1]: 30 each)
        assert all(bool(torch.isfinite(t).all()) for t in c.ref + c.ref32), c.name
    by = {c.name: c for c in AC.GAUSS_CASES}
    assert any(float(c.data[1][b].sum()) != c.kvo[b] for c in AC.GAUSS_CASES for b in range(len(c.kv)) if c.kv[b])
    assert not bool(by["A"].data[1][2].any()) and by["A"].kv[2] == 3                              # all-zero durations on valid tokens
    assert bool((by["F"].data[1][1, :4] == 30).all())
    cen = by["F"].data[1][1].cumsum(0) - by["F"].data[1][1] / 2
    assert float(-AC.GAUSS_DELTA * (0.0 - cen[3]) ** 2) < -104                                    # expf underflows to zero in f32
    for c in AC.GAUSS_IDENTITY:                                                                    # both identities fit the channels
        assert c.C == 65 and c.Tm <= c.C and c.To <= c.C
        hs, _, g = c.data
        assert float(hs.sum()) == len(c.kv) * c.Tm and float(g.sum()) == len(c.kv) * c.To


def test_gauss_refusals_come_before_any_launch(lib):
    keep, p, _ = _ragged(lib, 1)
    assert lib.jatts_gaussian_upsample_fwd(p, p, p, p, 1, 513, 8, 4, 0.1, p, p, None) == ERR_UNSUPPORTED and b"<= 512" in lib.jatts_last_error()
    assert lib.jatts_gaussian_upsample_bwd(p, p, p, p, p, 1, 513, 8, 4, 0.1, p, None) == ERR_UNSUPPORTED and b"<= 512" in lib.jatts_last_error()
    assert lib.jatts_gaussian_upsample_bwd(p, p, p, p, p, 1, 8, 0, 4, 0.1, p, None) == ERR_ARG and b"no frames" in lib.jatts_last_error()
    assert lib.jatts_gaussian_upsample_fwd(p, p, p, p, 1, 8, 0, 4, 0.1, p, p, None) == 0           # the forward has nothing to write
    del keep


def test_write_case_table():
    """profiles/alignment_cases.txt: kernel -> case -> structural class."""
    lines = ["# kernel  case  ->  structural class"]
    for tm, ti in AC.MAS_SHAPES + AC.MAS_LIMIT_SHAPES[:1]:
        c = AC.mas_class(tm, ti)
        lines.append(f"mas_kernel  ({tm}, {ti}) x {'/'.join(AC.MAS_KINDS)}  ->  W {c['W']}  slots {c['slots']}  T_mel%8 {c['mel_mod8']}  "
                     f"T_mel {c['order']} T_inp  ring rounds {c['ring_rounds']}  lds {c['lds']}")
    for n, group in enumerate(AC.mas_launches(AC.MAS_SHAPES)):
        lines.append(f"mas_kernel  launch {n}: {len(group)} sequences, priced {AC.mas_lds(max(t for t, _ in group), max(i for _, i in group))} bytes")
    for c in AC.ALIGN_BWD_CASES:
        k = c.classes()
        kern = "align_logp_kernel + bwd_frames + bwd_tokens" if c in AC.ALIGN_FWD_CASES else "bwd_frames + bwd_tokens"
        extra = "".join([f"  masked {c.masked}" if c.masked else "", f"  coincident {c.coincident}" if c.coincident else ""])
        lines.append(f"{kern}  {c.name} frames {c.flens} tokens {c.tlens} adim {c.adim} ld {c.ld}  ->  chunks {k['chunks']} tail {k['chunk_tail']}  "
                     f"nf {k['nf']}  lane strides {k['lane_strides']}  lds {k['lds']}  -inf fill {k['fill']}  token tiles {k['token_tiles']} tail "
                     f"{k['token_tail']}  frame chunk tail {k['frame_chunk_tail']}  T_f=0 {int(k['zero_frames'])}{extra}")
    for c in AC.GAUSS_CASES + AC.GAUSS_IDENTITY:
        k = c.classes()
        lines.append(f"gauss_up_fwd + gauss_up_bwd  {c.name} kv {c.kv} kvo {c.kvo} Tm {c.Tm} To {c.To} C {c.C}  ->  kv parity {k['kv_parity']}  "
                     f"K2%16 {k['k2_mod16']}  kvo%64 {k['frame_tail']}  To%64 {k['store_tail']}  To%32 {k['bwd_chunk_tail']}  padded token tiles "
                     f"{k['padded_tiles']}  partial {k['partial_tiles']}  wave passes {k['wave_passes']}  kv=0 {int(k['kv0'])}  kvo=0 {int(k['kvo0'])}")
    path = os.path.join(ROOT, "profiles", "alignment_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert os.path.getsize(path) < 1 << 20
