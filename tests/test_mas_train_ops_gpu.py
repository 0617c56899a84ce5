"""The differentiable halves of the MAS trainers' own kernels: masked Gaussian upsampling (jatts_gaussian_upsample_fwd / _bwd) and the gradient of
the alignment log-probabilities (jatts_alignment_logp_bwd).

References: float64 torch autograd on the CPU of the reference's expressions, restated here (modules/length_regulator.py:141-153 with the trainers'
masks; modules/alignments.py:50-60).  Yardstick: the float32 CPU autograd evaluation of the same expression, which is what the reference itself
computes -- each output's max abs error against float64 must be <= 4 x that evaluation's (summation order and expf differ; measured ratios per case
are in profiles/r11_notes.md)."""
import functools
import json

import pytest
import torch

from helpers import golden_state, load_golden

pytestmark = pytest.mark.gpu

FACTOR = 4.0
GAUSS_CASES = [((5, 17, 1), (40, 67, 3), 20), ((130, 64), (260, 131), 384), ((33, 64), (100, 97), 2 * 192)]
ALIGN_CASES = [((5, 17, 1), (40, 67, 3), 12), ((130, 64), (260, 131), 384)]


def _gauss_expr(hs, ds, ilens, olens, g, dtype, delta=0.1):
    """(out (B, To, C), d_hs (B, Tm, C)) of the masked Gaussian upsampling in `dtype` on the CPU, by autograd."""
    B, Tm, _ = hs.shape
    To = max(olens)
    h = hs.to(dtype).clone().requires_grad_(True)
    d = ds.to(dtype)
    tm = torch.arange(Tm).unsqueeze(0) < torch.tensor(ilens).unsqueeze(1)
    fm = (torch.arange(To).unsqueeze(0) < torch.tensor(olens).unsqueeze(1)).to(dtype)
    tpos = torch.arange(To).to(dtype).unsqueeze(0) * fm                      # padded frames sit at t = 0
    cen = d.cumsum(-1) - d / 2
    energy = -delta * (tpos.unsqueeze(-1) - cen.unsqueeze(1)) ** 2
    p = torch.softmax(energy.masked_fill(~tm.unsqueeze(1), float("-inf")), dim=2)
    out = torch.matmul(p, h)
    out.backward(g.to(dtype))
    return out.detach(), h.grad


@functools.lru_cache(maxsize=None)
def _gauss_case(ilens, olens, C):
    gen = torch.Generator().manual_seed(1000 + C + sum(ilens))
    B, Tm, To = len(ilens), max(ilens), max(olens)
    hs = torch.randn(B, Tm, C, generator=gen)
    ds = torch.randint(0, 7, (B, Tm), generator=gen).float()
    for b, n in enumerate(ilens):
        ds[b, n:] = 0.0
    ds[0, 0] = 0.0                                                            # a zero-duration token
    if float(ds[1].sum()) == olens[1]:                                        # one utterance whose durations do not add up to its frames
        ds[1, 0] += 1.0
    assert float(ds[1].sum()) != olens[1] and float(ds[0, 0]) == 0.0
    g = torch.randn(B, To, C, generator=gen)                                  # non-zero at padded frames too
    ref = _gauss_expr(hs, ds, ilens, olens, g, torch.float64)
    f32 = _gauss_expr(hs, ds, ilens, olens, g, torch.float32)
    return hs, ds, g, ref, f32


def _run_gauss(cuda, ilens, olens, hs, ds, g):
    from jatts_amd import hip
    B, Tm, To, C = len(ilens), max(ilens), max(olens), hs.shape[2]
    kv = torch.tensor(ilens, dtype=torch.int32, device=cuda)
    kvo = torch.tensor(olens, dtype=torch.int32, device=cuda)
    dsd = ds.to(cuda)
    out, stat = hip.gaussian_upsample_fwd(dsd, hs.reshape(B * Tm, C).to(cuda), kv, kvo, B, Tm, To, 0.1)
    dhs = hip.gaussian_upsample_bwd(dsd, stat, g.reshape(B * To, C).to(cuda), kv, kvo, B, Tm, To, 0.1)
    return out.view(B, To, C), dhs.view(B, Tm, C)


def _held(name, got, ref, f32):
    e = float((got.double().cpu() - ref).abs().max())
    e32 = float((f32.double() - ref).abs().max())
    print(f"{name}: max|err| {e:.3e}, f32 CPU {e32:.3e}, ratio {e / max(e32, 1e-300):.2f}")
    assert e <= FACTOR * e32, (name, e, e32)


@pytest.mark.parametrize("ilens,olens,C", GAUSS_CASES)
def test_gaussian_upsample_fwd_bwd(cuda, lib, ilens, olens, C):
    hs, ds, g, (ro, rd), (fo, fd) = _gauss_case(ilens, olens, C)
    out, dhs = _run_gauss(cuda, ilens, olens, hs, ds, g)
    _held(f"gauss out {ilens} C{C}", out, ro, fo)
    _held(f"gauss d_hs {ilens} C{C}", dhs, rd, fd)
    tol = FACTOR * float((fo.double() - ro).abs().max())
    for b, (n, no) in enumerate(zip(ilens, olens)):
        assert not dhs[b, n:].any(), "d_hs must be exactly zero at padded tokens"
        if no < max(olens):                                                   # padded frames: the t = 0 row of the float64 reference
            t0 = torch.softmax((-0.1 * (0.0 - (ds[b].double().cumsum(-1) - ds[b].double() / 2)) ** 2)[:n], dim=0) @ hs[b, :n].double()
            assert float((out[b, no:].double().cpu() - t0.unsqueeze(0)).abs().max()) <= tol


def _align_expr(ff, tf, ilens, dlp, dtype):
    """(d_feats (B, To, A), d_text (B, Tm, A)) of log_softmax_j(-||f_i - t_j||_2) with padded tokens masked, in `dtype` on the CPU, by autograd
    (one utterance at a time: the (To, Tm, A) difference tensor is the large object)."""
    dF, dT = [], []
    Tm = tf.shape[1]
    for b in range(ff.shape[0]):
        f = ff[b].to(dtype).clone().requires_grad_(True)
        t = tf[b].to(dtype).clone().requires_grad_(True)
        dist = torch.norm(f.unsqueeze(1) - t.unsqueeze(0), p=2, dim=2)
        mask = torch.arange(Tm) >= ilens[b]
        lp = torch.log_softmax((-dist).masked_fill(mask.unsqueeze(0), float("-inf")), dim=-1)
        lp.masked_fill(mask.unsqueeze(0), 0.0).backward(dlp[b].to(dtype).masked_fill(mask.unsqueeze(0), 0.0))
        dF.append(f.grad)
        dT.append(t.grad)
    return torch.stack(dF), torch.stack(dT)


@functools.lru_cache(maxsize=None)
def _align_case(ilens, olens, A):
    gen = torch.Generator().manual_seed(2000 + A + sum(ilens))
    B, Tm, To = len(ilens), max(ilens), max(olens)
    ff, tf = torch.randn(B, To, A, generator=gen), torch.randn(B, Tm, A, generator=gen)
    dlp = torch.randn(B, To, Tm, generator=gen)
    for b, n in enumerate(ilens):
        dlp[b, :, n:] = 1e3 * (1.0 + torch.rand(To, Tm - n, generator=gen))   # finite garbage at padded token columns
    return ff, tf, dlp, _align_expr(ff, tf, ilens, dlp, torch.float64), _align_expr(ff, tf, ilens, dlp, torch.float32)


def _run_align(cuda, ilens, olens, ff, tf, dlp):
    """Forward through the library (the saved log_p of autograd.AlignLogProb), then the new backward; d_text placed into the padded rows."""
    from jatts_amd import hip
    B, Tm, To, A = len(ilens), max(ilens), max(olens), ff.shape[2]
    rbf, rbv = hip.RaggedBatch([To] * B, cuda), hip.RaggedBatch(ilens, cuda)
    tsel = torch.tensor([b * Tm + i for b in range(B) for i in range(ilens[b])], device=cuda)
    f2, t2 = ff.reshape(B * To, A).to(cuda), tf.reshape(B * Tm, A).to(cuda).index_select(0, tsel).contiguous()
    lp = hip.alignment_logp(rbf, rbv, f2, t2, A)
    dl = torch.full((B * To, lp.shape[1]), 7.0, device=cuda)
    dl[:, :Tm] = dlp.reshape(B * To, Tm).to(cuda)
    dF, dTv = hip.alignment_logp_bwd(rbf, rbv, f2, t2, lp, dl)
    dT = torch.zeros(B * Tm, A, device=cuda).index_copy(0, tsel, dTv)
    return dF.view(B, To, A), dT.view(B, Tm, A)


@pytest.mark.parametrize("ilens,olens,A", ALIGN_CASES)
def test_alignment_logp_bwd(cuda, lib, ilens, olens, A):
    ff, tf, dlp, (rF, rT), (fF, fT) = _align_case(ilens, olens, A)
    dF, dT = _run_align(cuda, ilens, olens, ff, tf, dlp)
    _held(f"align d_feats {ilens} A{A}", dF, rF, fF)
    _held(f"align d_text {ilens} A{A}", dT, rT, fT)
    for b, n in enumerate(ilens):
        assert not dT[b, n:].any(), "d_text must be exactly zero at padded tokens"


def test_autograd_functions_match_the_entries(cuda, lib, monkeypatch):
    """autograd.GaussianUpsample / AlignLogProb (routed to its own kernel) run the same kernels: their gradients equal the direct calls bit for bit."""
    from jatts_amd import autograd as A
    monkeypatch.setitem(A.MAS_OWN_KERNELS, "align_bwd", True)
    ilens, olens, C = GAUSS_CASES[0]
    hs, ds, g, _, _ = _gauss_case(ilens, olens, C)
    B, Tm, To = len(ilens), max(ilens), max(olens)
    out, dhs = _run_gauss(cuda, ilens, olens, hs, ds, g)
    kv, kvo = torch.tensor(ilens, dtype=torch.int32, device=cuda), torch.tensor(olens, dtype=torch.int32, device=cuda)
    h = hs.reshape(B * Tm, C).to(cuda).requires_grad_(True)
    d = ds.to(cuda).requires_grad_(True)
    o = A.GaussianUpsample.apply(h, d, kv, kvo, B, Tm, To, 0.1)
    o.backward(g.reshape(B * To, C).to(cuda))
    assert torch.equal(o.detach().view(B, To, C), out) and torch.equal(h.grad.view(B, Tm, C), dhs) and d.grad is None
    ilens, olens, Ad = ALIGN_CASES[0]
    ff, tf, dlp, _, _ = _align_case(ilens, olens, Ad)
    dF, dT = _run_align(cuda, ilens, olens, ff, tf, dlp)
    f = ff.reshape(-1, Ad).to(cuda).requires_grad_(True)
    t = tf.reshape(-1, Ad).to(cuda).requires_grad_(True)
    lp = A.AlignLogProb.apply(f, t, len(ilens), list(ilens))
    lp.backward(dlp.to(cuda))
    assert torch.equal(f.grad.view_as(dF), dF) and torch.equal(t.grad.view_as(dT), dT)


def test_new_entries_are_deterministic(cuda, lib):
    ilens, olens, C = GAUSS_CASES[1]
    hs, ds, g, _, _ = _gauss_case(ilens, olens, C)
    a, b = _run_gauss(cuda, ilens, olens, hs, ds, g), _run_gauss(cuda, ilens, olens, hs, ds, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ilens, olens, A = ALIGN_CASES[1]
    ff, tf, dlp, _, _ = _align_case(ilens, olens, A)
    a, b = _run_align(cuda, ilens, olens, ff, tf, dlp), _run_align(cuda, ilens, olens, ff, tf, dlp)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _no_torch_arithmetic(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch.softmax / torch.matmul inside a MAS training step")
    monkeypatch.setattr(torch, "softmax", boom)
    monkeypatch.setattr(torch, "matmul", boom)


def _matcha_step():
    from jatts_amd.models import MatchaTTS_MAS
    from jatts_amd.models.matchatts_train import criterion
    from jatts_amd.synthetic import matcha_golden_tweaks
    z, keys = load_golden("matcha_mas_train_small.npz")
    zi, _ = load_golden("matcha_forward_small.npz")
    m = MatchaTTS_MAS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(matcha_golden_tweaks(golden_state(keys, 3)))
    m = m.to("cuda:0").train()
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")

    def step():
        m.zero_grad(set_to_none=True)
        ret = m(t("text"), il, t("feats"), ol, cfm_t=t("t"), cfm_noise=t("z"))
        losses = criterion(ret, None, il, duration_loss=True, olens=ol, forward_sum=True, bin_loss=True, lambda_align=2.0)
        losses["loss"].backward()
        return losses, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return step


def _vits_step():
    from jatts_amd.models import VITS
    from jatts_amd.models.vits_train import criterion
    z, keys = load_golden("vits_train_small.npz")
    zi, _ = load_golden("vits_forward_small.npz")
    m = VITS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(golden_state(keys, 2))
    m = m.to("cuda:0").train()
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")

    def step():
        m.zero_grad(set_to_none=True)
        ret = m(t("text"), il, t("feats"), ol, spembs=t("spembs"), post_noise=t("noise"))
        losses = criterion(ret, il, ol, duration_loss=True, forward_sum=True, bin_loss=True, lambda_align=2.0)
        losses["loss"].backward()
        return losses, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return step


def _routing():
    from jatts_amd import autograd as A
    return A.MAS_OWN_KERNELS


_STEPS = {"matcha_mas": _matcha_step, "vits": _vits_step}
_ROUTED = pytest.mark.xfail(condition=not all(_routing().values()), strict=True,
                            reason="autograd.MAS_OWN_KERNELS leaves a piece on the parent's sequence (torch.softmax + BMM / float64 torch.matmul): "
                                   "the routing rule and its timing table are in profiles/r11_notes.md")


@_ROUTED
@pytest.mark.parametrize("model", sorted(_STEPS))
def test_mas_step_has_no_torch_softmax_or_matmul(cuda, lib, monkeypatch, model):
    """One forward + criterion + backward AS THE TRAINERS ARE ROUTED, with torch.softmax and torch.matmul raising."""
    step = _STEPS[model]()
    _no_torch_arithmetic(monkeypatch)
    losses, _ = step()
    assert all(bool(torch.isfinite(v.detach()).all()) for v in losses.values())


@pytest.mark.parametrize("model", sorted(_STEPS))
def test_mas_step_on_own_kernels(cuda, lib, monkeypatch, model):
    """The same step with both pieces FORCED onto the own kernels: completes with torch.softmax / torch.matmul raising, finite, and agrees with the
    parent's sequences (forced the other way) -- every loss to 1e-5, every parameter's gradient norm by the check the reference pins of
    tests/test_training_gpu.py apply to a step: |norm - norm'| / max(norm', floor, 1e-3) <= 3e-3, floor = 1e-5 of the global gradient norm (gradients
    that are exactly zero in exact arithmetic -- conv biases in front of a batch-statistics BatchNorm -- are rounding noise of the global scale in BOTH
    paths, so they are compared as norms against that floor, not element by element)."""
    from jatts_amd import autograd as A
    step = _STEPS[model]()
    for k in A.MAS_OWN_KERNELS:
        monkeypatch.setitem(A.MAS_OWN_KERNELS, k, False)
    l0, g0 = step()
    for k in A.MAS_OWN_KERNELS:
        monkeypatch.setitem(A.MAS_OWN_KERNELS, k, True)
    _no_torch_arithmetic(monkeypatch)
    l1, g1 = step()
    assert all(bool(torch.isfinite(v.detach()).all()) for v in l1.values())
    for k in l0:
        a, b = float(l0[k].detach()), float(l1[k].detach())
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (k, a, b)
    floor = 1e-5 * float(torch.sqrt(sum((v.double() ** 2).sum() for v in g0.values())))
    assert g0.keys() == g1.keys()
    for n in g0:
        got, ref = float(g1[n].double().norm()), float(g0[n].double().norm())
        assert abs(got - ref) / max(ref, floor, 1e-3) <= 3e-3, (n, got, ref)


def test_text_longer_than_512_is_refused(cuda, lib):
    """Host-side argument checks: nothing is launched."""
    from jatts_amd import hip
    from jatts_amd._abi import JattsHipError
    B, Tm, To, C = 1, 513, 8, 4
    kv, kvo = torch.tensor([Tm], dtype=torch.int32, device=cuda), torch.tensor([To], dtype=torch.int32, device=cuda)
    ds, hs = torch.ones(B, Tm, device=cuda), torch.zeros(B * Tm, C, device=cuda)
    with pytest.raises(JattsHipError):
        hip.gaussian_upsample_fwd(ds, hs, kv, kvo, B, Tm, To)
    with pytest.raises(JattsHipError):
        hip.gaussian_upsample_bwd(ds, torch.zeros(B * To, 2, device=cuda), torch.zeros(B * To, C, device=cuda), kv, kvo, B, Tm, To)
    rbf, rbv = hip.RaggedBatch([To], cuda), hip.RaggedBatch([Tm], cuda)
    lp = torch.zeros(To, 520, device=cuda)
    with pytest.raises(JattsHipError):
        hip.alignment_logp_bwd(rbf, rbv, torch.zeros(To, C, device=cuda), torch.zeros(Tm, C, device=cuda), lp, lp.clone())
