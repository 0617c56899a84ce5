"""The training attention products on the fp32_bf16x3 arithmetic (round 10): jatts_bgemm_emul (the per-product bound, fp64 references over every tile,
edge and load path, batch indexing, determinism across tile variants, refusals), autograd.BMM under autograd.arithmetic(attention="fp32_bf16x3") and the whole train steps
of the four trainers with attention="fp32_bf16x3" and the routing forced on -- at the tolerances the existing tests apply to exact f32."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from helpers import golden_state, load_golden, maxdiff, relerr
from jatts_amd.synthetic import FS2_SMALL
from test_train_emul_gpu import PER_PRODUCT_7, _check_grads, _fs2_batch, _fs2_golden

pytestmark = pytest.mark.gpu

FORMS = [(False, False), (False, True), (True, False), (True, True)]


def _operands(g, O, I, m, n, k, ta, tb, dev):
    a = torch.randn(O, I, *((k, m) if ta else (m, k)), generator=g)
    b = torch.randn(O, I, *((n, k) if tb else (k, n)), generator=g)
    return a.to(dev), b.to(dev)


def _ref64(a, b, ta, tb):
    a, b = a.double().cpu(), b.double().cpu()
    return (a.transpose(-1, -2) if ta else a) @ (b.transpose(-1, -2) if tb else b)


@pytest.mark.parametrize("ta,tb", FORMS)
def test_bgemm_emul_per_product_bound(cuda, lib, ta, tb):
    """K = 1, M = 160, N = 96: every output is ONE product; random significands, exponents 2^-20 .. 2^20 (the generator of
    test_emulated_wgrad_per_product_bound): |c - a b| <= 2.01 x 2^-24 |a b| element by element.  alpha = 0.5 and accumulate onto zeros give exact
    multiples of that result: alpha is applied after the two accumulators are joined."""
    from jatts_amd import hip
    g = torch.Generator().manual_seed(7)
    M, N = 160, 96

    def rnd(n):
        m = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
        e = torch.randint(-20, 21, (n,), generator=g).double()
        s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        return (s * m * 2.0 ** e).float()
    av, bv = rnd(M), rnd(N)
    a = (av.view(1, 1, 1, M) if ta else av.view(1, 1, M, 1)).to(cuda)
    b = (bv.view(1, 1, N, 1) if tb else bv.view(1, 1, 1, N)).to(cuda)
    c = hip.bgemm(a, b, trans_a=ta, trans_b=tb, dtype=hip.F32E)
    prod = av.double().view(M, 1) * bv.double().view(1, N)
    ratio = ((c[0, 0].double().cpu() - prod).abs() / (prod.abs() * 2.0 ** -24)).max()
    print("per-product ratio", ta, tb, float(ratio))
    assert float(ratio) <= PER_PRODUCT_7
    half = hip.bgemm(a, b, trans_a=ta, trans_b=tb, alpha=0.5, dtype=hip.F32E)
    assert torch.equal(half, 0.5 * c)
    # accumulate: through the C entry (hip.bgemm always overwrites)
    acc = torch.zeros_like(c)
    lda, ldb = a.stride(2), b.stride(2)
    rc = lib.jatts_bgemm_emul(a.data_ptr(), 0, 0, lda, int(ta), b.data_ptr(), 0, 0, ldb, int(tb), acc.data_ptr(), 0, 0, N, 1, 1, M, N, 1, 0.5, 1, hip.F32E,
                              None)
    assert rc == 0, lib.jatts_last_error()
    torch.cuda.synchronize()
    assert torch.equal(acc, 0.5 * c)


SHAPES = [(2, 2, 130, 70, 33), (1, 3, 64, 192, 100), (1, 2, 200, 129, 258), (2, 1, 1, 1, 1), (1, 1, 70, 70, 70)]


@pytest.mark.parametrize("ta,tb", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bgemm_emul_against_float64(cuda, lib, shape, ta, tb):
    """M and N tile edges with a K tail | the 192-wide tile | two m tiles, n just past 128, K two past eight chunks | 1 x 1 x 1 | the element-load path
    (operands one element off a 16-byte boundary, ld % 4 != 0).  relerr <= 2e-6 (test_bgemm_and_bmm_function's bound for the exact kernel) for both kernels; where
    K >= 96 also max|emul - fp64| <= 2 max|exact-f32 kernel - fp64| on the same inputs (below that the exact kernel's error is a single rounding and
    the per-product bound above is the criterion)."""
    from jatts_amd import hip
    O, I, m, n, k = shape
    g = torch.Generator().manual_seed(sum(shape))
    if shape == (1, 1, 70, 70, 70):
        def off(r, c):      # a (r x c) matrix starting one element off a 16-byte boundary, leading dimension c + 1 (odd here or not, never 4 | ld with the offset)
            buf = torch.randn(r * (c + 1) + 8, generator=g).to(cuda)
            return buf[1:1 + r * (c + 1)].view(r, c + 1)[:, :c][None, None]
        a, b = off(*((k, m) if ta else (m, k))), off(*((n, k) if tb else (k, n)))
        assert a.data_ptr() % 16 != 0 and a.stride(2) % 4 != 0 and a.stride(3) == 1
    else:
        a, b = _operands(g, O, I, m, n, k, ta, tb, cuda)
    ref = _ref64(a, b, ta, tb)
    c = hip.bgemm(a, b, trans_a=ta, trans_b=tb, dtype=hip.F32E)
    cf = hip.bgemm(a, b, trans_a=ta, trans_b=tb)
    e_e, e_f = maxdiff(c.double().cpu(), ref), maxdiff(cf.double().cpu(), ref)
    print("bgemm_emul", shape, ta, tb, "relerr", relerr(c, ref), "max|emul - 64|", e_e, "max|f32 - 64|", e_f)
    assert c.shape == (O, I, m, n)
    assert relerr(c, ref) <= 2e-6
    assert relerr(cf, ref) <= 2e-6      # the exact partner is held to its own bound too: a wrong one would only make the comparison below easier
    if k >= 96:
        assert e_e <= 2.0 * e_f, (e_e, e_f)


def test_bgemm_emul_batch_indexing_and_determinism(cuda, lib):
    from jatts_amd import hip
    g = torch.Generator().manual_seed(11)
    O, I, m, n, k = 3, 2, 70, 48, 33
    a = torch.randn(O, I, m, k, generator=g).to(cuda)
    bs = torch.randn(I, n, k, generator=g).to(cuda)                 # shared over O: outer stride 0
    c = hip.bgemm(a, bs, trans_b=True, dtype=hip.F32E)
    ref = a.double().cpu() @ bs.double().cpu().transpose(-1, -2).unsqueeze(0)
    assert relerr(c, ref) <= 2e-6
    # permuted views with non-trivial batch strides, as the attention passes them: (B, T, H, d) -> (B, H, T, d)
    q = torch.randn(O, m, I, k, generator=g).to(cuda).permute(0, 2, 1, 3)
    kk = torch.randn(O, n, I, k, generator=g).to(cuda).permute(0, 2, 1, 3)
    assert not q.is_contiguous() and q.stride(3) == 1
    c2 = hip.bgemm(q, kk, trans_b=True, dtype=hip.F32E)
    assert relerr(c2, q.double().cpu() @ kk.double().cpu().transpose(-1, -2)) <= 2e-6
    out = torch.full((O, I, m, n), float("nan"), device=cuda)
    got = hip.bgemm(q, kk, trans_b=True, out=out, dtype=hip.F32E)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, c2)
    assert torch.equal(hip.bgemm(q, kk, trans_b=True, dtype=hip.F32E), c2)
    # one shape through different tile variants (WNF | MF << 4): n = 48 goes to the 64-wide tile; force 128- and 192-wide, 128 and 64 rows
    for tile in (2 | 2 << 4, 3 | 2 << 4, 3 | 1 << 4):
        assert torch.equal(hip.bgemm(q, kk, trans_b=True, dtype=hip.F32E, _tile=tile), c2), tile


def test_bgemm_emul_refusals(cuda, lib):
    from jatts_amd import hip
    a, b = torch.randn(1, 1, 8, 8).to(cuda), torch.randn(1, 1, 8, 8).to(cuda)
    with pytest.raises(ValueError):
        hip.bgemm(a, b, dtype=hip.F32E6)
    c = torch.empty(1, 1, 8, 8, device=cuda)

    def call(pa, k, arith):
        return lib.jatts_bgemm_emul(pa, 0, 0, 8, 0, b.data_ptr(), 0, 0, 8, 0, c.data_ptr(), 0, 0, 8, 1, 1, 8, 8, k, 1.0, 0, arith, None)
    assert call(a.data_ptr(), 8, hip.F32E6) != 0 and b"six-product" in lib.jatts_last_error()
    assert call(None, 8, hip.F32E) != 0 and b"null pointer" in lib.jatts_last_error()
    assert call(a.data_ptr(), 0, hip.F32E) != 0 and b"bad geometry" in lib.jatts_last_error()
    assert call(a.data_ptr(), 8, hip.F32E) == 0


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_bmm_under_emul_attention(cuda, lib, monkeypatch, trans_b, shared):
    """Routing forced on: output and both gradients against float64 autograd at 2e-6; a backward run after the context has exited still takes the emulated
    kernel (its results equal those of direct hip.bgemm(dtype=F32E) calls, and the launches are counted); with the context off BMM is today's BMM."""
    from jatts_amd import autograd, hip
    from jatts_amd.autograd import BMM, arithmetic, current_arithmetic
    from jatts_amd.precision import TrainArithmetic
    monkeypatch.setattr(autograd, "emul_bgemm_wins", lambda m, n, k: True)
    O, I, m, n, k = 2, 2, 70, 48, 33
    g = torch.Generator().manual_seed(5 + trans_b + 2 * shared)
    a = torch.randn(O, I, m, k, generator=g)
    b = torch.randn(*(() if shared else (O,)), I, *((n, k) if trans_b else (k, n)), generator=g)
    gy = torch.randn(O, I, m, n, generator=g)
    ar, br = a.double().requires_grad_(), b.double().requires_grad_()
    (ar @ (br.transpose(-1, -2) if trans_b else br)).backward(gy.double())
    ad, bd = a.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    calls = []
    real = hip.bgemm
    monkeypatch.setattr(hip, "bgemm", lambda *x, **kw: (calls.append(kw.get("dtype", hip.F32)), real(*x, **kw))[1])
    with arithmetic("fp32", attention="fp32_bf16x3"):
        y = BMM.apply(ad, bd, trans_b)
    assert current_arithmetic() == TrainArithmetic(hip.F32, hip.F32)
    y.backward(gy.to(cuda))                       # after the context: what forward decided
    assert calls == [hip.F32E] * 3, calls
    yr = (ar @ (br.transpose(-1, -2) if trans_b else br)).detach()
    errs = dict(y=relerr(y.detach(), yr), da=relerr(ad.grad, ar.grad), db=relerr(bd.grad, br.grad))
    print("BMM emul", trans_b, shared, errs)
    assert all(v <= 2e-6 for v in errs.values()), errs
    assert torch.equal(y.detach(), real(ad.detach(), bd.detach(), trans_b=trans_b, dtype=hip.F32E))
    # context off (patched rule or not): today's BMM, bit for bit
    del calls[:]
    a2, b2 = a.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    with arithmetic("fp32"):
        y2 = BMM.apply(a2, b2, trans_b)
    y2.backward(gy.to(cuda))
    assert calls == [hip.F32] * 3
    assert torch.equal(y2.detach(), real(a2.detach(), b2.detach(), trans_b=trans_b))
    dc = gy.to(cuda)
    assert torch.equal(a2.grad, real(dc, b2.detach(), trans_b=not trans_b))
    db = real(dc, a2.detach(), trans_a=True) if trans_b else real(a2.detach(), dc, trans_a=True)
    assert torch.equal(b2.grad, db.sum(0) if shared else db)


# ------------------------------------------------------------------------------------------ whole train steps, attention="fp32_bf16x3", routing forced on
@pytest.fixture
def forced(monkeypatch):
    from jatts_amd import autograd, hip
    monkeypatch.setattr(autograd, "emul_bgemm_wins", lambda m, n, k: True)
    seen = []
    real = hip.bgemm
    monkeypatch.setattr(hip, "bgemm", lambda *x, **kw: (seen.append(kw.get("dtype", hip.F32)), real(*x, **kw))[1])
    return seen


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_fastspeech2_train_step_with_emulated_attention(cuda, lib, forced, precision):
    """test_fastspeech2_train_step_matches_reference's fixture and tolerances (outputs and losses 2e-5, gradient norms and sampled gradients 2e-3, total norm
    1e-3, the Adam-update bound) with every attention product on the emulated kernel."""
    from jatts_amd import hip
    from jatts_amd.models import FastSpeech2
    from jatts_amd.models.fastspeech2_train import criterion
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import FastSpeech2Trainer
    z, zi, keys, cfg = _fs2_golden()
    m = FastSpeech2(idim=20, **{**FS2_SMALL, **cfg})
    sd0 = golden_state(keys, 0)
    m.load_state_dict(sd0)
    m = m.to(cuda)
    batch = _fs2_batch(zi)
    il, ol = batch["ilens"], batch["olens"]
    with pytest.raises(ValueError, match="fp32_bf16x3"):
        FastSpeech2Trainer(m, attention="bf16")
    tr = FastSpeech2Trainer(m, lr=0.0008, grad_norm=1.0, warmup_steps=4000, precision=precision, attention="fp32_bf16x3")
    assert tr.attention == "fp32_bf16x3" and tr.precision == precision
    m.train()
    with arithmetic(precision, attention="fp32_bf16x3"):
        ret = m(batch["xs"], il, batch["ys"], ol, batch["durations"], il, batch["pitch"], il, batch["energys"], il)
        for k in ("before_outs", "after_outs", "d_outs", "p_outs", "e_outs"):
            assert relerr(ret[k].detach(), z["ref_" + k]) <= 2e-5, (k, relerr(ret[k].detach(), z["ref_" + k]))
        losses = criterion(ret, batch["durations"], batch["pitch"], batch["energys"], il)
        for k in ("mel_loss", "duration_loss", "pitch_loss", "energy_loss"):
            assert abs(float(losses[k]) - float(z[k])) <= 2e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k]), float(z[k]))
    losses["loss"].backward()
    assert forced and all(c == hip.F32E for c in forced), forced
    names = json.loads(str(z["grad_names"]))
    P = dict(m.named_parameters())
    for n, ref_norm in zip(names, z["grad_norms"]):
        assert abs(float(P[n].grad.norm()) - ref_norm) / max(ref_norm, 1e-3) <= 2e-3, (n, float(P[n].grad.norm()), ref_norm)
    for f in z.files:
        if f.startswith("grad:"):
            assert relerr(P[f[5:]].grad, z[f]) <= 2e-3, (f, relerr(P[f[5:]].grad, z[f]))
    tot = math.sqrt(sum(float(P[n].grad.double().pow(2).sum()) for n in names))
    assert abs(tot - float(z["total_grad_norm"])) <= 1e-3 * float(z["total_grad_norm"])
    m2 = FastSpeech2(idim=20, **{**FS2_SMALL, **cfg})
    m2.load_state_dict(sd0)
    m2 = m2.to(cuda)
    tr = FastSpeech2Trainer(m2, lr=0.0008, grad_norm=1.0, warmup_steps=4000, precision=precision, attention="fp32_bf16x3")
    del forced[:]
    out = tr.train_step(batch)
    assert forced and all(c == hip.F32E for c in forced)
    ev = tr.eval_step(batch)
    assert math.isfinite(float(ev["loss"]))
    assert abs(float(out["grad_norm"]) - float(z["total_grad_norm"])) <= 1e-3 * float(z["total_grad_norm"])
    P2 = dict(m2.named_parameters())
    for f in z.files:
        if f.startswith("after:"):
            n = f[6:]
            before, after_ref, after = sd0[n].double(), torch.tensor(z[f]).double(), P2[n].detach().cpu().double()
            step_ref, step = after_ref - before, after - before
            tol = 0.05 * tr.last_lr + 2.0 * float(before.abs().max()) * 2.0 ** -23
            assert float((step - step_ref).abs().max()) <= tol, (n, float((step - step_ref).abs().max()), tol)
            assert float(step.abs().max()) > 0.5 * tr.last_lr


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
@pytest.mark.parametrize("which", ["tts1", "mas"])
def test_matcha_train_step_with_emulated_attention(cuda, lib, forced, which, precision):
    """test_matcha_tts1 / test_matcha_mas_train_step_matches_reference: same fixtures, same tolerances (d_outs 2e-5, losses 3e-5, gradients 3e-3)."""
    from jatts_amd import hip
    from jatts_amd.models import MatchaTTS, MatchaTTS_MAS
    from jatts_amd.models.matchatts_train import criterion
    from jatts_amd.synthetic import matcha_golden_tweaks
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import MatchaTTSTrainer
    tts1 = which == "tts1"
    z, keys = load_golden("matcha_tts1_train_small.npz" if tts1 else "matcha_mas_train_small.npz")
    zi, _ = load_golden("matcha_tts1_forward_small.npz" if tts1 else "matcha_forward_small.npz")
    m = (MatchaTTS if tts1 else MatchaTTS_MAS)(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(matcha_golden_tweaks(golden_state(keys, 4 if tts1 else 3)))
    m = m.to(cuda).train()
    assert MatchaTTSTrainer(m, precision=precision, attention="fp32_bf16x3").attention == "fp32_bf16x3"
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    with arithmetic(precision, attention="fp32_bf16x3"):
        if tts1:
            ret = m(t("text"), il, t("feats"), ol, t("durations"), il, cfm_t=t("t"), cfm_noise=t("z"))
            assert relerr(ret["d_outs"].detach(), z["ref_d_outs"]) <= 2e-5
            losses = criterion(ret, t("durations"), il)
            names = ("cfm_loss", "encoder_prior_loss", "duration_loss")
        else:
            ret = m(t("text"), il, t("feats"), ol, cfm_t=t("t"), cfm_noise=t("z"))
            assert torch.equal(ret["ds"].cpu(), torch.tensor(z["ref_ds"]))
            losses = criterion(ret, None, il, duration_loss=True, olens=ol, forward_sum=True, bin_loss=True, lambda_align=2.0)
            names = ("cfm_loss", "encoder_prior_loss", "duration_loss", "forward_sum_loss", "bin_loss")
        for k in names:
            assert abs(float(losses[k].detach()) - float(z[k])) <= 3e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k].detach()), float(z[k]))
    losses["loss"].backward()
    assert forced and all(c == hip.F32E for c in forced), forced
    _check_grads(m, z, 3e-3)


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_vits_train_step_with_emulated_attention(cuda, lib, forced, precision):
    """test_vits_train_step_matches_reference: same fixture, same tolerances."""
    from jatts_amd import hip
    from jatts_amd.models import VITS
    from jatts_amd.models.vits_train import criterion
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import VITSTrainer
    z, keys = load_golden("vits_train_small.npz")
    zi, _ = load_golden("vits_forward_small.npz")
    m = VITS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(golden_state(keys, 2))
    m = m.to(cuda).train()
    assert VITSTrainer(m, precision=precision, attention="fp32_bf16x3").attention == "fp32_bf16x3"
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    with arithmetic(precision, attention="fp32_bf16x3"):
        ret = m(t("text"), il, t("feats"), ol, spembs=t("spembs"), post_noise=t("noise"))
        assert torch.equal(ret["ds"].cpu(), torch.tensor(z["ref_ds"]))
        losses = criterion(ret, il, ol, duration_loss=True, forward_sum=True, bin_loss=True, lambda_align=2.0)
        for k in ("mel_loss", "kl_loss", "duration_loss", "forward_sum_loss", "bin_loss"):
            assert abs(float(losses[k].detach()) - float(z[k])) <= 3e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k].detach()), float(z[k]))
    losses["loss"].backward()
    assert forced and all(c == hip.F32E for c in forced), forced
    _check_grads(m, z, 3e-3, floor=1e-5 * float(np.sqrt((z["grad_norms"] ** 2).sum())))


def test_graph_mode_replays_the_same_training_with_emulated_attention(cuda, lib, forced):
    """The trainers of test_graph_mode_replays_the_same_training_in_fp32_bf16x3 with the attention products emulated too: the graph trainer's eager first
    step and its three captured / replayed steps are bit-identical to four eager steps -- losses, gradients and parameters."""
    from jatts_amd import hip
    from jatts_amd.models import FastSpeech2
    from jatts_amd.training import FastSpeech2Trainer
    z, zi, keys, cfg = _fs2_golden()
    batch = _fs2_batch(zi)

    def make():
        m = FastSpeech2(idim=20, **{**FS2_SMALL, "stop_gradient_from_pitch_predictor": True, "use_masking": True})
        m.load_state_dict(golden_state(keys, 0))
        return m.to(cuda)
    kw = dict(lr=1e-3, grad_norm=1.0, warmup_steps=10, precision="fp32_bf16x3", attention="fp32_bf16x3")
    a, b = FastSpeech2Trainer(make(), **kw), FastSpeech2Trainer(make(), capture_graph=True, **kw)
    for step in range(4):      # the graph trainer: eager, then capture + replay, replay, replay
        la, lb = a.train_step(batch), b.train_step(batch)
        print("graph step", step, {k: (float(la[k]), float(lb[k])) for k in ("loss", "grad_norm")}, "max|dg|", maxdiff(a.flat_g, b.flat_g))
        for k in ("loss", "mel_loss", "duration_loss", "pitch_loss", "energy_loss"):
            assert float(la[k]) == float(lb[k]), (step, k, float(la[k]), float(lb[k]))
        assert torch.equal(a.flat_g, b.flat_g) and torch.equal(a.flat_p, b.flat_p), step
    (st,) = b._graphs.values()
    assert st["graph"] is not None
    assert forced and all(c == hip.F32E for c in forced)


def test_default_attention_is_untouched(cuda, lib, monkeypatch):
    """attention=None with the routing patched to True: one FastSpeech2 step's losses and every gradient are torch.equal to a step taken with the
    arithmetic context never entered -- and no emulated launch happens."""
    from jatts_amd import autograd, hip
    from jatts_amd.models import FastSpeech2
    from jatts_amd.training import FastSpeech2Trainer
    z, zi, keys, cfg = _fs2_golden()
    batch = _fs2_batch(zi)

    def make():
        m = FastSpeech2(idim=20, **{**FS2_SMALL, **cfg})
        m.load_state_dict(golden_state(keys, 0))
        return m.to(cuda)
    # never entered: the step's pieces by hand, without train_step's contexts
    ref = FastSpeech2Trainer(make(), lr=0.0008, grad_norm=1.0, warmup_steps=4000)
    hip.zero_pool_begin(cuda)
    try:
        lr_ = ref._train_step(batch)
    finally:
        hip.zero_pool_end()
    monkeypatch.setattr(autograd, "emul_bgemm_wins", lambda m, n, k: True)
    seen = []
    real = hip.bgemm
    monkeypatch.setattr(hip, "bgemm", lambda *x, **kw: (seen.append(kw.get("dtype", hip.F32)), real(*x, **kw))[1])
    for att in (None, "fp32"):
        tr = FastSpeech2Trainer(make(), lr=0.0008, grad_norm=1.0, warmup_steps=4000, attention=att)
        out = tr.train_step(batch)
        assert seen and all(c == hip.F32 for c in seen)
        for k in lr_:
            assert torch.equal(out[k], lr_[k]), (att, k)
        assert torch.equal(tr.flat_g, ref.flat_g) and torch.equal(tr.flat_p, ref.flat_p)
