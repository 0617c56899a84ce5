#!/usr/bin/env python3
"""jatts_bgemm against torch.matmul (rocBLAS) on the attention products of the FastSpeech2 training step (batch 32 x 2 heads, T = 768, d_k = 192).
    python tools/bench_bgemm.py [--T 770]      (T % 4 != 0: the T x T operand takes the element-load path)
    python tools/bench_bgemm.py --emul         exact jatts_bgemm against jatts_bgemm_emul (hip.bgemm(dtype=hip.F32E)), timed ALTERNATELY over --rounds
                                               rounds: FastSpeech2's four products at T = 768 and 770, the Matcha decoder blocks (2 heads x 256) and the
                                               Gaussian-upsampling product; prints min / median per kernel, the exact kernel's run-to-run spread and the
                                               ratio of the medians"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from jatts_amd import hip  # noqa: E402


def t(fn, it=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it


def emul_table(dev, rounds):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    B = 32
    cases = []
    for T in (768, 770):
        q, k, p = r(B, 2, T, 192), r(B, 2, T, 192), r(B, 2, T, T)
        cases += [(f"fs2 T={T} q k^T  NT m{T} n{T} k192", q, k, False, True), (f"fs2 T={T} P v    NN m{T} n192 k{T}", p, k, False, False),
                  (f"fs2 T={T} dS^T q TN m{T} n192 k{T}", p, q, True, False), (f"fs2 T={T} dP v^T NT m{T} n{T} k192", q, k, False, True)]
    for T in (768, 384):      # Matcha decoder transformer blocks: 2 heads x 256 at the full and the down-sampled frame rate
        q, k, p = r(B, 2, T, 256), r(B, 2, T, 256), r(B, 2, T, T)
        cases += [(f"matcha T={T} q k^T NT m{T} n{T} k256", q, k, False, True), (f"matcha T={T} P v   NN m{T} n256 k{T}", p, k, False, False),
                  (f"matcha T={T} dS^T q TN m{T} n256 k{T}", p, q, True, False)]
    pu, hs = r(B, 1, 768, 192), r(B, 1, 192, 384)      # Gaussian upsampling p_up @ hs: frames x tokens x adim
    cases += [("upsample p_up hs NN m768 n384 k192", pu, hs, False, False), ("upsample d hs    TN m192 n384 k768", pu, r(B, 1, 768, 384), True, False)]
    print(f"{'product':40s} {'exact min':>9s} {'med':>8s} {'spread':>7s} | {'emul min':>9s} {'med':>8s} | exact/emul (medians)   TFLOP/s exact, emul")
    for name, a, b, ta, tb in cases:
        m = a.shape[-1] if ta else a.shape[-2]
        kk = a.shape[-2] if ta else a.shape[-1]
        n = b.shape[-2] if tb else b.shape[-1]
        fl = 2.0 * a.shape[0] * a.shape[1] * m * n * kk
        te, tm = [], []
        for _ in range(rounds):
            te.append(t(lambda: hip.bgemm(a, b, trans_a=ta, trans_b=tb), 5))
            tm.append(t(lambda: hip.bgemm(a, b, trans_a=ta, trans_b=tb, dtype=hip.F32E), 5))
        te.sort()
        tm.sort()
        me, mm = te[len(te) // 2], tm[len(tm) // 2]
        print(f"{name:40s} {te[0] * 1e3:9.1f} {me * 1e3:8.1f} {100 * (te[-1] - te[0]) / te[0]:6.1f}% | {tm[0] * 1e3:9.1f} {mm * 1e3:8.1f} | {me / mm:6.3f}"
              f"                 {fl / me / 1e9:6.1f} {fl / mm / 1e9:6.1f}", flush=True)


def main():
    dev = torch.device("cuda:0")
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=768)
    ap.add_argument("--emul", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.emul:
        return emul_table(dev, args.rounds)
    B, H, T, dk = 32, 2, args.T, 192
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, H, T, dk, generator=g).to(dev)
    k = torch.randn(B, H, T, dk, generator=g).to(dev)
    p = torch.randn(B, H, T, T, generator=g).to(dev)
    cases = [("q k^T   (T x T x d_k, NT)", lambda: hip.bgemm(q, k, trans_b=True), lambda: torch.matmul(q, k.transpose(-1, -2)), 2.0 * B * H * T * T * dk),
             ("P v     (T x d_k x T, NN)", lambda: hip.bgemm(p, k), lambda: torch.matmul(p, k), 2.0 * B * H * T * T * dk),
             ("dS^T q  (T x d_k x T, TN)", lambda: hip.bgemm(p, q, trans_a=True), lambda: torch.matmul(p.transpose(-1, -2), q), 2.0 * B * H * T * T * dk),
             ("dO v^T  (T x T x d_k, NT)", lambda: hip.bgemm(q, k, trans_b=True), lambda: torch.matmul(q, k.transpose(-1, -2)), 2.0 * B * H * T * T * dk)]
    for name, f1, f2, fl in cases:
        a, b = t(f1), t(f2)
        print(f"{name:40s} jatts_bgemm {a * 1e3:7.1f} us {fl / a / 1e9:6.1f} TFLOP/s   torch.matmul {b * 1e3:7.1f} us {fl / b / 1e9:6.1f} TFLOP/s")


if __name__ == "__main__":
    main()
