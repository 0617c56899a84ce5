"""The alignment-learning kernels (jatts_mas_viterbi, jatts_alignment_logp, jatts_alignment_logp_bwd, jatts_gaussian_upsample_fwd / _bwd) at every
tile edge, tie and length limit of alignment_cases.py, against exact or float64 CPU references.  test_alignment_cases_cpu.py proves without a GPU
that the tables reach every structural class; profiles/alignment_cases.txt lists them; the measured figures are in profiles/r31_notes.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import alignment_cases as AC
from oracle.mas_oracle import monotonic_alignment_search

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- MAS
def _mas_run(cuda, mats):
    """One ragged launch: ld = round_up(max T_inp, 8), NaN in the padding.  -> per sequence (path, dur, score)."""
    from jatts_amd import hip
    fl, tl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    lp = torch.full((sum(fl), hip.round_up(max(tl), 8)), float("nan"))
    o = 0
    for m in mats:
        lp[o:o + m.shape[0], :m.shape[1]] = torch.from_numpy(m)
        o += m.shape[0]
    path, dur, score = hip.mas_viterbi(hip.RaggedBatch(fl, cuda), hip.RaggedBatch(tl, cuda), lp.to(cuda))
    path, dur, score = path.cpu().numpy(), dur.cpu().numpy(), score.cpu().numpy()
    out, o, ot = [], 0, 0
    for b, m in enumerate(mats):
        out.append((path[o:o + m.shape[0]], dur[ot:ot + m.shape[1]], float(score[b])))
        o, ot = o + m.shape[0], ot + m.shape[1]
    return out


@functools.lru_cache(maxsize=None)
def _mas_want(kind, tm, ti):
    return monotonic_alignment_search(AC.mas_input(kind, tm, ti)[1])


def _mas_check(kind, shape, got, want):
    lp = AC.mas_input(kind, *shape)[1]
    path, dur, score = got
    assert np.array_equal(path, want), (kind, shape, int((path != want).sum()))
    assert np.array_equal(dur, np.bincount(path, minlength=shape[1]))
    s = float(lp[np.arange(shape[0]), want].astype(np.float64).sum())
    assert abs(score - s) <= 1e-9 * max(1.0, abs(s)), (kind, shape, score, s)


@pytest.mark.parametrize("kind", AC.MAS_KINDS)
def test_mas_every_edge_and_tie(cuda, lib, kind):
    """Paths, durations and scores against the float64 oracle (and, for the exact kinds, the real reference's stored paths) in ragged launches, and
    the first, middle and last sequence of every launch once more alone."""
    fix = AC.mas_fixture() if kind in AC.MAS_EXACT else {}
    for group in AC.mas_launches(AC.MAS_SHAPES):
        got = _mas_run(cuda, [AC.mas_input(kind, *s)[1] for s in group])
        for s, g in zip(group, got):
            _mas_check(kind, s, g, _mas_want(kind, *s))
            if (kind,) + s in fix:
                assert np.array_equal(g[0], fix[(kind,) + s][1]), (kind, s)
        for n in sorted({0, len(group) // 2, len(group) - 1}):
            (alone,) = _mas_run(cuda, [AC.mas_input(kind, *group[n])[1]])
            assert np.array_equal(alone[0], got[n][0]) and np.array_equal(alone[1], got[n][1]) and alone[2] == got[n][2], (kind, group[n])


@pytest.mark.parametrize("shape", AC.MAS_LIMIT_SHAPES)
def test_mas_at_the_lds_limit(cuda, lib, shape):
    """The largest launches the kernel's LDS holds (163 804 and 163 732 of 163 808 bytes), one workgroup each."""
    assert AC.mas_lds(*shape) <= AC.MAS_LDS_MAX < AC.mas_lds(shape[0] + 1, shape[1])
    (got,) = _mas_run(cuda, [AC.mas_input("q4", *shape)[1]])
    _mas_check("q4", shape, got, _mas_want("q4", *shape))


# ---------------------------------------------------------------- alignment log-probabilities, forward
def _i32(cuda, v):
    return torch.tensor(v, dtype=torch.int32, device=cuda)


def _align_fwd(cuda, lib, case, only=None):
    """jatts_alignment_logp into a NaN-filled (rows + 3 guard rows, ld) buffer.  only=b: utterance b ALONE, as a one-sequence batch whose row and
    token offsets point into the full arrays, so that every other utterance's rows must come back untouched."""
    from jatts_amd import _abi, hip
    feats, text, _ = case.data
    rows = sum(case.flens)
    out = torch.full((rows + 3, case.ld), float("nan"), device=cuda)
    fl, tl = case.flens, case.tlens
    cuf, cut = np.concatenate([[0], np.cumsum(fl)]).tolist(), np.concatenate([[0], np.cumsum(tl)]).tolist()
    if only is not None:
        cuf, cut, fl, tl = cuf[only:only + 2], cut[only:only + 2], fl[only:only + 1], tl[only:only + 1]
    cu_f, cu_t = _i32(cuda, cuf), _i32(cuda, cut)
    f, t = feats.to(cuda), text.to(cuda)
    rg = _abi.Ragged(cu_f.data_ptr(), len(fl), max(fl), 1, 0, None)
    _abi.check(lib.jatts_alignment_logp(C.byref(rg), cu_t.data_ptr(), max(tl), f.data_ptr(), t.data_ptr(), case.adim, out.data_ptr(), case.ld,
                                        hip._stream()), "jatts_alignment_logp")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", AC.ALIGN_FWD_CASES, ids=repr)
def test_alignment_logp_forward(cuda, lib, case):
    got = _align_fwd(cuda, lib, case)
    rows = sum(case.flens)
    assert bool(got[rows:].isnan().all()), "rows behind the batch were written"
    worst = 0.0
    for b, fs, _ in case.utterances():
        tl = case.tlens[b]
        if fs.stop == fs.start:
            continue
        ref, f32 = case.ref[0][b], case.ref32[0][b]
        err = (got[fs, :tl].double() - ref).abs()
        e32 = float((f32.double() - ref).abs().max())
        ratio = float((err / case.fwd_bound(b)).max())
        worst = max(worst, ratio)
        print(f"align fwd {case.name}[{b}] frames {case.flens[b]} tokens {tl} adim {case.adim}: max|err| {float(err.max()):.3e}, f32 CPU {e32:.3e}, "
              f"ratio {float(err.max()) / max(e32, 1e-300):.2f}, max err/bound {ratio:.3f}")
        assert bool(torch.isinf(got[fs, tl:]).all()) and bool((got[fs, tl:] < 0).all()), "columns T_t <= i < ld must be -inf"
    for b, fs, _ in case.utterances():          # an utterance alone: the same rows bit for bit, everybody else's untouched
        if len(case.flens) == 1 or fs.stop == fs.start:
            continue
        alone = _align_fwd(cuda, lib, case, only=b)
        assert torch.equal(alone[fs], got[fs]), (case.name, b)
        mask = torch.ones(rows + 3, dtype=torch.bool)
        mask[fs] = False
        assert bool(alone[mask].isnan().all()), (case.name, b, "rows of other utterances were written")
    assert worst <= 1.0, (case.name, worst)


# ---------------------------------------------------------------- alignment log-probabilities, backward
def _align_bwd(cuda, case):
    """The saved log_p from the library's forward (cut to the case's ld: 17 columns in the training form, as autograd.AlignLogProb builds it), the
    case's masked columns set to -inf, then the backward."""
    from jatts_amd import hip
    feats, text, dlp = case.data
    rbf, rbt = hip.RaggedBatch(case.flens, cuda), hip.RaggedBatch(case.tlens, cuda)
    f, t = feats.to(cuda), text.to(cuda)
    lp = hip.alignment_logp(rbf, rbt, f, t, case.adim)[:, :case.ld].contiguous()
    for b, fs, _ in case.utterances():
        for j in case.masked.get(b, []):
            lp[fs, j] = float("-inf")
    dF, dT = hip.alignment_logp_bwd(rbf, rbt, f, t, lp, dlp.to(cuda))
    return dF, dT


@pytest.mark.parametrize("case", AC.ALIGN_BWD_CASES, ids=repr)
def test_alignment_logp_backward(cuda, lib, case):
    dF, dT = _align_bwd(cuda, case)
    _, _, rF, rT = case.ref
    _, _, fF, fT = case.ref32
    AC.held(f"align bwd {case.name} d_feats", dF, rF, fF)
    AC.held(f"align bwd {case.name} d_text", dT, rT, fT)
    dTc = dT.cpu()
    for b, fs, ts in case.utterances():
        if fs.stop == fs.start:
            assert not bool(dTc[ts].any()), "an utterance without frames: d_text exactly zero"
        for j in case.masked.get(b, []):
            assert not bool(dTc[ts][j].any()), "a masked column: d_text exactly zero"
    again = _align_bwd(cuda, case)
    assert torch.equal(again[0], dF) and torch.equal(again[1], dT), "two launches must be bit-identical"


def test_both_backward_paths_of_align_logprob_hold_the_masked_column_contract(cuda, lib):
    """autograd.AlignLogProb has two backward paths (MAS_OWN_KERNELS["align_bwd"]): the kernel and the float64 torch form.  On a saved log_p with -inf
    columns inside the valid tokens both must give what plain autograd of masked_fill(-inf) -> log_softmax gives: no gradient to the masked token,
    its dlog_p still in sum_j g.  (Uniform frames: the torch form works on the padded batch.)"""
    from jatts_amd import autograd as A
    case = AC.AlignCase("masked-padded", [20, 20], [33, 9], 65, ld=33, masked={0: [5, 31], 1: [3, 4]}, seed=13)
    feats, text, dlp = case.data
    _, _, rF, rT = case.ref
    _, _, fF, fT = case.ref32
    dF, dT = _align_bwd(cuda, case)
    AC.held("align bwd masked-padded kernel d_feats", dF, rF, fF)
    AC.held("align bwd masked-padded kernel d_text", dT, rT, fT)
    B, To, Tm = 2, 20, 33
    tsel = torch.tensor([b * Tm + i for b in range(B) for i in range(case.tlens[b])], device=cuda)
    tf = torch.zeros(B * Tm, case.adim, device=cuda).index_copy(0, tsel, text.to(cuda))
    valid = torch.arange(Tm, device=cuda).unsqueeze(0) < torch.tensor(case.tlens, device=cuda).unsqueeze(1)
    f = feats.to(cuda)
    # the torch form trusts the VALUES of the saved log_p (the kernel only its -inf marks), so it gets what a caller that masks before the log-softmax
    # would have saved: the reference's log_p, normalised over the unmasked columns
    lp = torch.full((B, To, Tm), float("-inf"))
    for b in range(B):
        lp[b, :, :case.tlens[b]] = case.ref[0][b].float()
    lp = lp.to(cuda)
    dF64, dT64 = A.AlignLogProb._backward_f64(f, tf, lp, valid, dlp.to(cuda).view(B, To, Tm), B)
    dT64v = dT64.index_select(0, tsel)
    AC.held("align bwd masked-padded f64 form d_feats", dF64, rF, fF)
    AC.held("align bwd masked-padded f64 form d_text", dT64v, rT, fT)
    for b, _, ts in case.utterances():
        for j in case.masked[b]:
            assert not bool(dT[ts][j].any()) and not bool(dT64v[ts][j].any())


# ---------------------------------------------------------------- Gaussian upsampling
def _gauss_run(cuda, case):
    from jatts_amd import hip
    hs, ds, g = case.data
    B, Tm, To, Cc = len(case.kv), case.Tm, case.To, case.C
    kv, kvo = _i32(cuda, case.kv), _i32(cuda, case.kvo)
    dsd = ds.to(cuda)
    out, stat = hip.gaussian_upsample_fwd(dsd, hs.reshape(B * Tm, Cc).to(cuda), kv, kvo, B, Tm, To, AC.GAUSS_DELTA)
    dhs = hip.gaussian_upsample_bwd(dsd, stat, g.reshape(B * To, Cc).to(cuda), kv, kvo, B, Tm, To, AC.GAUSS_DELTA)
    return out.view(B, To, Cc), dhs.view(B, Tm, Cc)


@pytest.mark.parametrize("case", AC.GAUSS_CASES, ids=repr)
def test_gaussian_upsample_edges(cuda, lib, case):
    out, dhs = _gauss_run(cuda, case)
    (ro, rd), (fo, fd) = case.ref, case.ref32
    AC.held(f"gauss {case.name} out", out, ro, fo)
    AC.held(f"gauss {case.name} d_hs", dhs, rd, fd)
    tol = AC.FACTOR * float((fo.double() - ro).abs().max()) + 4 * AC.U * float(ro.abs().max())
    hs, ds, _ = case.data
    oc, dc = out.cpu(), dhs.cpu()
    for b, (n, no) in enumerate(zip(case.kv, case.kvo)):
        assert not bool(dc[b, n:].any()), "d_hs must be exactly zero at padded tokens"
        if n == 0:
            assert not bool(oc[b].any()), "an utterance without tokens: zero rows"
        elif no < case.To:                        # padded frames: the t = 0 row of the float64 reference
            d = ds[b, :n].double()
            t0 = torch.softmax(-AC.GAUSS_DELTA * (0.0 - (d.cumsum(-1) - d / 2)) ** 2, dim=0) @ hs[b, :n].double()
            assert float((oc[b, no:].double() - t0.unsqueeze(0)).abs().max()) <= tol
    again = _gauss_run(cuda, case)
    assert torch.equal(again[0], out) and torch.equal(again[1], dhs), "two launches must be bit-identical"


@pytest.mark.parametrize("case", AC.GAUSS_IDENTITY, ids=repr)
def test_gaussian_backward_recomputes_the_forward_weights_bit_for_bit(cuda, lib, case):
    """hs = identity on the first Tm channels: out[b, f, j] is the forward's p[b, f, j] exactly (one non-zero product per sum on the f32 matrix pipe);
    g = identity on the first To channels: d_hs[b, j, f] is the backward's recomputed p[b, f, j].  The file's central claim: they are the same bits."""
    out, dhs = _gauss_run(cuda, case)
    pf, pb = out[:, :, :case.Tm], dhs[:, :, :case.To].transpose(1, 2)
    assert torch.equal(pf, pb), int((pf != pb).sum())
    p = pf.cpu()
    for b, n in enumerate(case.kv):               # and they are weights: rows sum to 1 over the valid tokens, nothing at the padded ones
        assert not bool(p[b, :, n:].any()) and float((p[b].double().sum(-1) - 1).abs().max()) <= 64 * AC.U
    assert not bool(out[:, :, case.Tm:].any()) and not bool(dhs[:, :, case.To:].any())
