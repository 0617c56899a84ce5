"""Training on the fp32_bf16x3 arithmetic (round 7): the device packer of the emulated conv operand (bit for bit the host packing), the emulated
weight-gradient kernel (fp64 references, the per-product bound, ragged boundaries, determinism), Conv1dFunction's third mode and the whole
`_train_step` of the four trainers on the real reference's goldens under precision="fp32_bf16x3" -- at the tolerances the existing tests apply to fp32."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden_state, load_golden, maxdiff, relerr
from jatts_amd.synthetic import FS2_SMALL

pytestmark = pytest.mark.gpu

PER_PRODUCT_7 = 2.01      # x 2^-24 |dy x|: dropped w2 v1 + w2 v2 (<= 2^-24 + 2^-32) plus the one add that joins the two accumulators (2^-24); DESIGN §4


def _special_weight(n, c, k, seed):
    """random values with exact zeros, +-2^-100 and all-24-significand-bits-set values sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, c, k, generator=g)
    flat = w.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)
    q = max(1, flat.numel() // 8)
    flat[idx[:q]] = 0.0
    flat[idx[q:2 * q:2]] = 2.0 ** -100
    flat[idx[q + 1:2 * q:2]] = -(2.0 ** -100)
    full = torch.tensor([(2.0 - 2.0 ** -23) * 2.0 ** e for e in (-30, -3, 0, 5, 40)])     # 0x..7fffff significands
    m = idx[2 * q:3 * q]
    flat[m] = full[torch.arange(m.numel()) % full.numel()] * torch.where(torch.arange(m.numel()) % 2 == 0, 1.0, -1.0)
    return w


@pytest.mark.parametrize("n,c,k", [(96, 80, 3), (1, 256, 1), (384, 1, 1), (64, 64, 5), (33, 17, 4), (384, 1536, 3), (1536, 384, 1)])
def test_emul_weight_packer_on_the_device_equals_the_host_packing(cuda, lib, n, c, k):
    from jatts_amd import hip
    w = _special_weight(n, c, k, n + c + k).to(cuda)
    assert bool((w == 0).any()) and bool((w.abs() == 2.0 ** -100).any())
    got, c_pad = hip.pack_conv_weight_bf16x3_dev(w)
    ref = hip.pack_conv_weight_bf16x3_k32(w, 64)
    assert c_pad == hip.round_up(c, 64) and got.dtype == torch.bfloat16 and got.numel() == ref.numel()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    got, c_pad = hip.pack_conv_weight_bf16x3_dev(w, dgrad=True)
    ref = hip.pack_conv_weight_bf16x3_k32(w.permute(1, 0, 2).flip(2).contiguous(), 64)
    assert c_pad == hip.round_up(n, 64) and torch.equal(got.view(torch.int16), ref.view(torch.int16))


def _wgrad_ref64(x, dy, lens, k, dil, pad):
    """dW, db in fp64, one utterance at a time (zero padding at utterance boundaries)"""
    x, dy = x.double().cpu(), dy.double().cpu()
    n_out, c_in = dy.shape[1], x.shape[1]
    dw = torch.zeros(n_out, c_in, k, dtype=torch.float64)
    o = 0
    for L in lens:
        xs, ds = x[o:o + L], dy[o:o + L]
        for tap in range(k):
            sh = tap * dil - pad
            lo, hi = max(0, -sh), min(L, L - sh)
            if hi > lo:
                dw[:, :, tap] += ds[lo:hi].t() @ xs[lo + sh:hi + sh]
        o += L
    return dw, dy.sum(0)


@pytest.mark.parametrize("c_in,n_out,k,dil,lens", [(64, 96, 3, 1, [70, 5, 33]), (80, 64, 5, 2, [40, 41]), (128, 128, 1, 1, [129]),
                                                   (48, 20, 7, 3, [64, 30]), (192, 320, 5, 1, [300, 257, 64, 1]), (384, 200, 3, 1, [768, 500])])
def test_conv1d_backward_in_the_emulated_mode_matches_autograd(cuda, lib, c_in, n_out, k, dil, lens):
    """test_conv1d_backward_matches_autograd's shapes and seeds through Conv1dFunction under arithmetic("fp32_bf16x3"): y, dx, dW, db within the exact-f32 path's
    2e-5 of fp64 autograd; the emulated weight-gradient kernel itself (whatever the trainer's shape rule routes) held to the same 2e-5 and to
    max|dW_emul - dW_64| <= 2 max|dW_f32 - dW_64| (acceptance rule (3) of DESIGN §4, against the existing exact-f32 kernel)."""
    from jatts_amd import hip
    from jatts_amd.autograd import Conv1dFunction, arithmetic
    g = torch.Generator().manual_seed(c_in + n_out + k)
    R = sum(lens)
    x = torch.randn(R, c_in, generator=g)
    w = torch.randn(n_out, c_in, k, generator=g) / math.sqrt(c_in * k)
    b = torch.randn(n_out, generator=g) * 0.1
    gy = torch.randn(R, n_out, generator=g)
    pad = (k - 1) // 2 * dil
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    outs, o = [], 0
    for n in lens:
        outs.append(F.conv1d(xr[o:o + n].t().unsqueeze(0), wr, br, padding=pad, dilation=dil)[0].t())
        o += n
    yr = torch.cat(outs)
    yr.backward(gy.double())
    xd, wd, bd = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_(), b.to(cuda).requires_grad_()
    rb = hip.RaggedBatch(lens, cuda)
    with arithmetic("fp32_bf16x3"):
        y = Conv1dFunction.apply(xd, wd, bd, rb, dil, pad)
        y.backward(gy.to(cuda))
    errs = dict(y=relerr(y.detach(), yr.detach()), dx=relerr(xd.grad, xr.grad), dw=relerr(wd.grad, wr.grad), db=relerr(bd.grad, br.grad))
    print("emul mode", (c_in, n_out, k, dil), errs)
    assert all(v <= 2e-5 for v in errs.values()), errs
    # the kernel itself, beside the exact-f32 kernel on the same inputs
    dw_e, db_e = hip.conv1d_wgrad(rb, x.to(cuda), gy.to(cuda), c_in, n_out, k, dil, pad, want_db=True, dtype=hip.F32E)
    dw_f = hip.conv1d_wgrad(rb, x.to(cuda), gy.to(cuda), c_in, n_out, k, dil, pad)
    e_e, e_f = maxdiff(dw_e.double().cpu(), wr.grad), maxdiff(dw_f.double().cpu(), wr.grad)
    print("wgrad kernel", (c_in, n_out, k, dil), "relerr", relerr(dw_e, wr.grad), "max|emul - 64|", e_e, "max|f32 - 64|", e_f)
    assert relerr(dw_e, wr.grad) <= 2e-5 and relerr(db_e, br.grad) <= 2e-5
    assert e_e <= 2.0 * e_f, (e_e, e_f)


@pytest.mark.parametrize("k,dil", [(1, 1), (3, 1), (5, 2)])
def test_emulated_wgrad_per_product_bound(cuda, lib, k, dil):
    """K_eff = 1: one row, so every dW[n][c][centre tap] is ONE product dy[n] x[c]: random significands, exponents 2^-20 .. 2^20;
    |dW - dy x| <= 2.01 x 2^-24 |dy x| element by element (PER_PRODUCT["7"]); the other taps see only zero padding."""
    from jatts_amd import hip
    g = torch.Generator().manual_seed(7 + k)
    n_out, c_in = 160, 96

    def rnd(n):
        m = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
        e = torch.randint(-20, 21, (n,), generator=g).double()
        s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
        return (s * m * 2.0 ** e).float()
    x, dy = rnd(c_in).view(1, c_in), rnd(n_out).view(1, n_out)
    pad = (k - 1) // 2 * dil
    rb = hip.RaggedBatch([1], cuda)
    dw = hip.conv1d_wgrad(rb, x.to(cuda), dy.to(cuda), c_in, n_out, k, dil, pad, dtype=hip.F32E).double().cpu()
    prod = dy.double().t() @ x.double()
    centre = (k - 1) // 2
    ratio = ((dw[:, :, centre] - prod).abs() / (prod.abs() * 2.0 ** -24)).max()
    print("per-product ratio", k, dil, float(ratio))
    assert float(ratio) <= PER_PRODUCT_7
    for tap in range(k):
        if tap != centre:
            assert float(dw[:, :, tap].abs().max()) == 0.0


@pytest.mark.parametrize("lens", [[300, 257, 64, 1], [1, 1, 1]])
def test_emulated_wgrad_ragged_boundaries_and_determinism(cuda, lib, lens):
    """k = 5, dil = 2: the fp64 per-utterance reference (nothing leaks across utterance boundaries); two calls are bit-identical."""
    from jatts_amd import hip
    g = torch.Generator().manual_seed(len(lens))
    c_in, n_out, k, dil = 192, 320, 5, 2
    pad = (k - 1) // 2 * dil
    R = sum(lens)
    x, dy = torch.randn(R, c_in, generator=g), torch.randn(R, n_out, generator=g)
    rb = hip.RaggedBatch(lens, cuda)
    dw1, db1 = hip.conv1d_wgrad(rb, x.to(cuda), dy.to(cuda), c_in, n_out, k, dil, pad, want_db=True, dtype=hip.F32E)
    dw2, db2 = hip.conv1d_wgrad(rb, x.to(cuda), dy.to(cuda), c_in, n_out, k, dil, pad, want_db=True, dtype=hip.F32E)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    rw, rbias = _wgrad_ref64(x, dy, lens, k, dil, pad)
    # f32 result of a sum of R terms of size ~1: a few 2^-24 sqrt(R) of absolute error; 2e-5 relative to the tensor's scale as everywhere in this suite
    print("ragged", lens, relerr(dw1, rw), relerr(db1, rbias))
    assert relerr(dw1, rw) <= 2e-5 and relerr(db1, rbias) <= 2e-5
    # a leak across a boundary would be an O(1) error in an edge tap: element-wise, against the sum of |terms| (R of them, each ~1)
    assert maxdiff(dw1.double().cpu(), rw) <= 1e-5 * math.sqrt(max(R, 1)) * 4.0


def test_emulated_wgrad_refuses_the_six_product_code_and_falls_back_beyond_its_taps(cuda, lib):
    from jatts_amd import _abi, hip
    import ctypes as C
    g = torch.Generator().manual_seed(3)
    lens, c_in, n_out = [64, 30], 48, 20
    x, dy = torch.randn(sum(lens), c_in, generator=g).to(cuda), torch.randn(sum(lens), n_out, generator=g).to(cuda)
    rb = hip.RaggedBatch(lens, cuda)
    got = hip.conv1d_wgrad(rb, x, dy, c_in, n_out, 7, 3, 9, dtype=hip.F32E)          # k = 7: through the exact-f32 entry
    assert torch.equal(got, hip.conv1d_wgrad(rb, x, dy, c_in, n_out, 7, 3, 9))
    dw = torch.empty(n_out, c_in, 3, device=cuda)
    ws = torch.empty(2 * (3 * 64 * 64 + 64), device=cuda)
    rg = rb.struct(1)
    rc = lib.jatts_conv1d_wgrad_emul(C.byref(rg), x.data_ptr(), c_in, dy.data_ptr(), n_out, c_in, n_out, 3, 1, 1, hip.F32E6, dw.data_ptr(), None,
                                     ws.data_ptr(), None, None)
    assert rc != 0 and b"six-product" in lib.jatts_last_error()
    assert _abi is not None


# ------------------------------------------------------------------------------------------ whole train steps, precision="fp32_bf16x3"
def _fs2_golden():
    z, keys = load_golden("fs2_train_small.npz")
    zi, _ = load_golden("fs2_forward_small.npz")
    return z, zi, keys, json.loads(str(z["config"]))


def _fs2_batch(zi):
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    return dict(xs=t("text"), ilens=il, ys=t("feats"), olens=ol, durations=t("durations"), duration_lens=il, pitch=t("pitch"),
                pitch_lens=il, energys=t("energy"), energy_lens=il)


def test_fastspeech2_train_step_matches_reference_in_fp32_bf16x3(cuda, lib):
    """test_fastspeech2_train_step_matches_reference with precision="fp32_bf16x3": same fixture, same tolerances (outputs and losses 2e-5, gradient norms and
    sampled full gradients 2e-3, total norm 1e-3, the Adam-update bound)."""
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
    tr = FastSpeech2Trainer(m, lr=0.0008, grad_norm=1.0, warmup_steps=4000, precision="fp32_bf16x3")
    m.train()
    with arithmetic("fp32_bf16x3"):
        ret = m(batch["xs"], il, batch["ys"], ol, batch["durations"], il, batch["pitch"], il, batch["energys"], il)
        for k in ("before_outs", "after_outs", "d_outs", "p_outs", "e_outs"):
            assert relerr(ret[k].detach(), z["ref_" + k]) <= 2e-5, (k, relerr(ret[k].detach(), z["ref_" + k]))
        losses = criterion(ret, batch["durations"], batch["pitch"], batch["energys"], il)
        for k in ("mel_loss", "duration_loss", "pitch_loss", "energy_loss"):
            assert abs(float(losses[k]) - float(z[k])) <= 2e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k]), float(z[k]))
        losses["loss"].backward()
    names = json.loads(str(z["grad_names"]))
    P = dict(m.named_parameters())
    for n, ref_norm in zip(names, z["grad_norms"]):
        g = P[n].grad
        assert g is not None, n
        assert abs(float(g.norm()) - ref_norm) / max(ref_norm, 1e-3) <= 2e-3, (n, float(g.norm()), ref_norm)
    for f in z.files:
        if f.startswith("grad:"):
            assert relerr(P[f[5:]].grad, z[f]) <= 2e-3, (f, relerr(P[f[5:]].grad, z[f]))
    tot = math.sqrt(sum(float(P[n].grad.double().pow(2).sum()) for n in names))
    assert abs(tot - float(z["total_grad_norm"])) <= 1e-3 * float(z["total_grad_norm"])
    B = dict(m.named_buffers())
    for f in z.files:
        if f.startswith("buf:"):
            assert relerr(B[f[4:]], z[f]) <= 2e-5, f
    m2 = FastSpeech2(idim=20, **{**FS2_SMALL, **cfg})
    m2.load_state_dict(sd0)
    m2 = m2.to(cuda)
    tr = FastSpeech2Trainer(m2, lr=0.0008, grad_norm=1.0, warmup_steps=4000, precision="fp32_bf16x3")
    out = tr.train_step(batch)
    assert abs(tr.last_lr - float(z["lr_step1"])) <= 1e-12
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


def _check_grads(m, z, tol, floor=0.0):
    P = dict(m.named_parameters())
    names = json.loads(str(z["grad_names"]))
    assert [n for n, _ in m.named_parameters()] == names
    for n, ref_norm in zip(names, z["grad_norms"]):
        assert P[n].grad is not None, n
        assert abs(float(P[n].grad.norm()) - ref_norm) / max(ref_norm, floor, 1e-3) <= tol, (n, float(P[n].grad.norm()), ref_norm)
    for f in z.files:
        if f.startswith("grad:"):
            assert relerr(P[f[5:]].grad, z[f]) <= tol, (f, relerr(P[f[5:]].grad, z[f]))


def test_matcha_tts1_train_step_matches_reference_in_fp32_bf16x3(cuda, lib):
    """test_matcha_tts1_train_step_matches_reference under the emulated conv mode: same fixture, same tolerances (d_outs 2e-5, losses 3e-5, gradients 3e-3)."""
    from jatts_amd.models import MatchaTTS
    from jatts_amd.models.matchatts_train import criterion
    from jatts_amd.synthetic import matcha_golden_tweaks
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import MatchaTTSTrainer
    z, keys = load_golden("matcha_tts1_train_small.npz")
    zi, _ = load_golden("matcha_tts1_forward_small.npz")
    m = MatchaTTS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(matcha_golden_tweaks(golden_state(keys, 4)))
    m = m.to(cuda).train()
    assert MatchaTTSTrainer(m, precision="fp32_bf16x3").precision == "fp32_bf16x3"
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    with arithmetic("fp32_bf16x3"):
        ret = m(t("text"), il, t("feats"), ol, t("durations"), il, cfm_t=t("t"), cfm_noise=t("z"))
        assert relerr(ret["d_outs"].detach(), z["ref_d_outs"]) <= 2e-5
        losses = criterion(ret, t("durations"), il)
        for k in ("cfm_loss", "encoder_prior_loss", "duration_loss"):
            assert abs(float(losses[k]) - float(z[k])) <= 3e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k]), float(z[k]))
        losses["loss"].backward()
    _check_grads(m, z, 3e-3)


def test_matcha_mas_train_step_matches_reference_in_fp32_bf16x3(cuda, lib):
    """test_matcha_mas_train_step_matches_reference under the emulated conv mode: same fixture, same tolerances."""
    from jatts_amd.models import MatchaTTS_MAS
    from jatts_amd.models.matchatts_train import criterion
    from jatts_amd.synthetic import matcha_golden_tweaks
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import MatchaTTSTrainer
    z, keys = load_golden("matcha_mas_train_small.npz")
    zi, _ = load_golden("matcha_forward_small.npz")
    m = MatchaTTS_MAS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(matcha_golden_tweaks(golden_state(keys, 3)))
    m = m.to(cuda).train()
    assert MatchaTTSTrainer(m, precision="fp32_bf16x3").precision == "fp32_bf16x3"
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    with arithmetic("fp32_bf16x3"):
        ret = m(t("text"), il, t("feats"), ol, cfm_t=t("t"), cfm_noise=t("z"))
        assert torch.equal(ret["ds"].cpu(), torch.tensor(z["ref_ds"]))
        losses = criterion(ret, None, il, duration_loss=True, olens=ol, forward_sum=True, bin_loss=True, lambda_align=2.0)
        for k in ("cfm_loss", "encoder_prior_loss", "duration_loss", "forward_sum_loss", "bin_loss"):
            assert abs(float(losses[k].detach()) - float(z[k])) <= 3e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k].detach()), float(z[k]))
        losses["loss"].backward()
    _check_grads(m, z, 3e-3)


def test_vits_train_step_matches_reference_in_fp32_bf16x3(cuda, lib):
    """test_vits_train_step_matches_reference under the emulated conv mode: same fixture, same tolerances."""
    from jatts_amd.models import VITS
    from jatts_amd.models.vits_train import criterion
    from jatts_amd.autograd import arithmetic
    from jatts_amd.training import VITSTrainer
    z, keys = load_golden("vits_train_small.npz")
    zi, _ = load_golden("vits_forward_small.npz")
    m = VITS(idim=20, **json.loads(str(z["config"])))
    m.load_state_dict(golden_state(keys, 2))
    m = m.to(cuda).train()
    assert VITSTrainer(m, precision="fp32_bf16x3").precision == "fp32_bf16x3"
    t = lambda k: torch.tensor(zi[k])  # noqa: E731
    il, ol = t("text_lengths"), t("feats_lengths")
    with arithmetic("fp32_bf16x3"):
        ret = m(t("text"), il, t("feats"), ol, spembs=t("spembs"), post_noise=t("noise"))
        assert torch.equal(ret["ds"].cpu(), torch.tensor(z["ref_ds"]))
        losses = criterion(ret, il, ol, duration_loss=True, forward_sum=True, bin_loss=True, lambda_align=2.0)
        for k in ("mel_loss", "kl_loss", "duration_loss", "forward_sum_loss", "bin_loss"):
            assert abs(float(losses[k].detach()) - float(z[k])) <= 3e-5 * max(1.0, abs(float(z[k]))), (k, float(losses[k].detach()), float(z[k]))
        losses["loss"].backward()
    _check_grads(m, z, 3e-3, floor=1e-5 * float(np.sqrt((z["grad_norms"] ** 2).sum())))


def test_graph_mode_replays_the_same_training_in_fp32_bf16x3(cuda, lib):
    """The check of test_graph_mode_replays_the_same_training with precision="fp32_bf16x3" on both trainers: eager and captured / replayed steps agree step
    by step, also when the data changes under the same signature."""
    from jatts_amd.models import FastSpeech2
    from jatts_amd.training import FastSpeech2Trainer
    z, zi, keys, cfg = _fs2_golden()
    batch = _fs2_batch(zi)

    def make():
        m = FastSpeech2(idim=20, **{**FS2_SMALL, "stop_gradient_from_pitch_predictor": True, "use_masking": True})
        m.load_state_dict(golden_state(keys, 0))
        return m.to(cuda)
    a = FastSpeech2Trainer(make(), lr=1e-3, grad_norm=1.0, warmup_steps=10, precision="fp32_bf16x3")
    b = FastSpeech2Trainer(make(), lr=1e-3, grad_norm=1.0, warmup_steps=10, capture_graph=True, precision="fp32_bf16x3")
    g = torch.Generator().manual_seed(0)
    for step in range(6):
        cur = dict(batch)
        if step >= 3:
            cur["ys"] = batch["ys"] + 0.1 * torch.randn(batch["ys"].shape, generator=g)
            cur["pitch"] = batch["pitch"] + 0.1 * torch.randn(batch["pitch"].shape, generator=g)
        la, lb = a.train_step(cur), b.train_step(cur)
        for k in ("loss", "mel_loss", "duration_loss", "pitch_loss", "energy_loss", "grad_norm"):
            tol = 2e-5 * (1 + 5 * step)
            assert abs(float(la[k]) - float(lb[k])) <= tol * max(1.0, abs(float(la[k]))), (step, k, float(la[k]), float(lb[k]))
        assert a.steps == b.steps == step + 1 and a.last_lr == b.last_lr
        assert maxdiff(a.flat_g, b.flat_g) <= 2e-5 * (1 + 5 * step), (step, maxdiff(a.flat_g, b.flat_g))
        o = 0
        for p_ in a.params:
            k = p_.numel()
            if float(a.flat_g[o:o + k].abs().max()) > 1e-4:
                assert maxdiff(a.flat_p[o:o + k], b.flat_p[o:o + k]) <= 5e-6 * (1 + 5 * step), (step, o)
            o += k
    (st,) = b._graphs.values()
    assert st["graph"] is not None


def test_fastspeech2_training_reduces_the_loss_in_fp32_bf16x3(cuda, lib):
    """Twelve steps with dropout on, as test_fastspeech2_training_reduces_the_loss asks, under precision="fp32_bf16x3"."""
    from jatts_amd.models import FastSpeech2
    from jatts_amd.training import FastSpeech2Trainer
    z, zi, keys, cfg = _fs2_golden()
    m = FastSpeech2(idim=20, **{**FS2_SMALL, "stop_gradient_from_pitch_predictor": True, "use_masking": True})
    m.load_state_dict(golden_state(keys, 0))
    m = m.to(cuda)
    batch = _fs2_batch(zi)
    tr = FastSpeech2Trainer(m, lr=2e-3, grad_norm=1.0, warmup_steps=0, precision="fp32_bf16x3")
    hist = [float(tr.train_step(batch)["loss"]) for _ in range(12)]
    assert all(math.isfinite(v) for v in hist)
    assert min(hist[-3:]) < 0.8 * hist[0], hist
