#!/usr/bin/env python3
"""The MAS trainers' own Gaussian-upsampling and alignment-backward kernels against the op sequences they replace, timed ALTERNATELY on one box.
    python tools/bench_mas_ops.py [--rounds 7]
old = the sequence of the trainers before round 11, restated here: tpos / cen / energy / masked_fill / torch.softmax + autograd.BMM (jatts_bgemm) forward and
backward for the upsampling; the float64 torch.matmul form for the alignment backward.  new = autograd.GaussianUpsample / hip.alignment_logp_bwd.
Recipe sizes: B 32, Tm 128, To 768; C 384 (Matcha: adim) and 2 x 192 (VITS: the statistics width); alignment width A = adim 384.
Prints per case the largest difference between the two paths' gradients, min / median of both over --rounds samples (a sample = 200 calls behind 10
warm-ups), the spread (max - min) / min between the old path's own samples and new / old of the medians.  Both closures hold what a step would launch: the
old alignment backward its float64 casts, the new one the zeros + index_copy scatter of d_text into the padded rows; the upsampling rows time forward +
backward through autograd."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from jatts_amd import autograd as A  # noqa: E402
from jatts_amd import hip  # noqa: E402


def t(fn, it=200, warm=10):
    """Mean time of one call over a window of `it` calls behind `warm` untimed ones (device events): the ops are of the order of 100 us, so a sample is
    some tens of milliseconds of work, not a handful of launches."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it


def old_upsample(hs, ds, tm_, fm, B, Tm, To, C):
    tpos = torch.arange(To, device=hs.device).float().unsqueeze(0) * fm
    cen = ds.cumsum(-1) - ds / 2
    energy = -0.1 * (tpos.unsqueeze(-1) - cen.unsqueeze(1)) ** 2
    p_up = torch.softmax(energy.masked_fill(~tm_.unsqueeze(1), float("-inf")), dim=2)
    return A.BMM.apply(p_up.unsqueeze(1), hs.view(B, 1, Tm, C), False).squeeze(1).reshape(B * To, C)


def old_align_bwd(ff, tf, lp, valid, dlp, B):
    To, Tm, A_ = ff.shape[0] // B, tf.shape[0] // B, ff.shape[1]
    vm = valid.unsqueeze(1)
    g = dlp.double().masked_fill(~vm, 0.0)
    dscore = g - torch.exp(lp.double()) * g.sum(-1, keepdim=True)
    F_, T_ = ff.view(B, To, A_).double(), tf.view(B, Tm, A_).double()
    d2 = (F_ * F_).sum(-1).unsqueeze(2) + (T_ * T_).sum(-1).unsqueeze(1) - 2.0 * torch.matmul(F_, T_.transpose(1, 2))
    w = (-dscore / torch.sqrt(d2.clamp_min(1e-24))).masked_fill(~vm, 0.0)
    dF = w.sum(-1, keepdim=True) * F_ - torch.matmul(w, T_)
    wF = torch.matmul(w.transpose(1, 2), torch.cat([F_, torch.ones(B, To, 1, dtype=F_.dtype, device=F_.device)], dim=-1))
    dT = wF[..., A_:] * T_ - wF[..., :A_]
    return dF.reshape(B * To, A_).float(), dT.reshape(B * Tm, A_).float()


def row(name, old, new, rounds):
    to, tn = [], []
    for _ in range(rounds):
        to.append(t(old))
        tn.append(t(new))
    to.sort()
    tn.sort()
    mo, mn = to[len(to) // 2], tn[len(tn) // 2]
    print(f"{name:44s} old min {to[0] * 1e3:8.1f} med {mo * 1e3:8.1f} us (spread {100 * (to[-1] - to[0]) / to[0]:5.1f}%) | new min {tn[0] * 1e3:8.1f} "
          f"med {mn * 1e3:8.1f} us | new / old {mn / mo:6.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    B, Tm, To = 32, 128, 768
    ilens = [Tm - (3 * b) % 40 for b in range(B)]
    olens = [To - (17 * b) % 200 for b in range(B)]
    kv, kvo = hip.h2d(ilens, torch.int32, dev), hip.h2d(olens, torch.int32, dev)
    tm_ = torch.arange(Tm, device=dev).unsqueeze(0) < kv.unsqueeze(1)
    fm = (torch.arange(To, device=dev).unsqueeze(0) < kvo.unsqueeze(1)).float()
    ds = torch.zeros(B, Tm)
    for b in range(B):      # integer durations that add up to the utterance's frames
        cut = torch.sort(torch.randint(0, olens[b] + 1, (ilens[b] - 1,), generator=gen)).values
        ds[b, : ilens[b]] = torch.diff(torch.cat([torch.zeros(1, dtype=torch.int64), cut, torch.tensor([olens[b]])])).float()
    ds = ds.to(dev)
    for name, C in (("upsample fwd + bwd, Matcha C 384", 384), ("upsample fwd + bwd, VITS C 2 x 192", 2 * 192)):
        hs = torch.randn(B * Tm, C, generator=gen).to(dev).requires_grad_(True)
        g = torch.randn(B * To, C, generator=gen).to(dev)

        def old():
            hs.grad = None
            old_upsample(hs, ds, tm_, fm, B, Tm, To, C).backward(g)

        def new():
            hs.grad = None
            A.GaussianUpsample.apply(hs, ds, kv, kvo, B, Tm, To, 0.1).backward(g)

        old()
        go = hs.grad.clone()
        new()
        print(f"{name}: max |d_hs new - old| {float((hs.grad - go).abs().max()):.3e} (max |d_hs| {float(go.abs().max()):.3e})")
        row(name, old, new, args.rounds)
    Ad = 384
    ff, tf = torch.randn(B * To, Ad, generator=gen).to(dev), torch.randn(B * Tm, Ad, generator=gen).to(dev)
    dlp = torch.randn(B, To, Tm, generator=gen).to(dev)
    rbf, rbv = hip.RaggedBatch([To] * B, dev), hip.RaggedBatch(ilens, dev)
    tsel = hip.h2d([b * Tm + i for b in range(B) for i in range(ilens[b])], torch.int64, dev)
    lp = A.AlignLogProb.apply(ff, tf, B, ilens, tsel, tm_)
    tv = tf.index_select(0, tsel).contiguous()

    def new_align():
        dF, dTv = hip.alignment_logp_bwd(rbf, rbv, ff, tv, lp, dlp)
        return dF, torch.zeros_like(tf).index_copy(0, tsel, dTv)

    (oF, oT), (nF, nT) = old_align_bwd(ff, tf, lp, tm_, dlp, B), new_align()
    print(f"alignment backward: max |d_feats new - old| {float((nF - oF).abs().max()):.3e} (max {float(oF.abs().max()):.3e}), "
          f"max |d_text new - old| {float((nT - oT).abs().max()):.3e} (max {float(oT.abs().max()):.3e})")
    row("alignment backward, A 384", lambda: old_align_bwd(ff, tf, lp, tm_, dlp, B), new_align, args.rounds)


if __name__ == "__main__":
    main()
