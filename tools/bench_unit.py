#!/usr/bin/env python3
"""Micro-benchmark of the fused HiFi-GAN dilation-unit kernel at bench-sized shapes.
    python tools/bench_unit.py [--C 128 --k 11 --dil 1 --iters 10] [--all] [--variant 0|1|2 | --variants]
Prints avg ms, TFLOP/s and algorithmic GB/s per shape (HIP events on the launch stream).  --variants (emulated units): the windowed and the sliding
form of every shape side by side (jatts_resunit_desc.variant 1 / 2).  --single: the SINGLE-CONV unit (w2 = None; HiFi-GAN V3 shapes) against the two-conv unit of
the same shape, alternating rounds in one process, with the share of the binding roof."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from jatts_amd import hip  # noqa: E402


LAYOUT = [1]      # emulated units: 1 = the v_mfma_f32_16x16x32_bf16 kernels (the product form), 0 = the 32 x 32 x 16 ones (--layout 0)


def run(C, k, d, rate, iters, B=64, T=768, dtype=hip.F16, variant=0):
    dev = torch.device("cuda:0")
    rb = hip.RaggedBatch([T] * B, dev)
    rows = B * T * rate
    tdt = hip.torch_dtype(dtype)
    g = torch.Generator(device="cpu").manual_seed(0)
    x = (torch.randn(rows, C, generator=g) * 0.5).to(dev).to(tdt)
    y = torch.empty_like(x)
    wa, wb = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev), (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev)
    kw = {}
    if dtype == hip.F32S:
        (w1, i1), (w2, i2) = hip.pack_conv_weight_split(wa, 32), hip.pack_conv_weight_split(wb, 32)
        kw["ws"] = (i1, i2)
    elif dtype in hip.EMUL:
        if LAYOUT[0]:
            w1, w2 = hip.pack_unit_weight_bf16x3_k32(wa), hip.pack_unit_weight_bf16x3_k32(wb)
            kw["w_layout"] = 1
            kw["variant"] = variant
        else:
            w1, w2 = hip.pack_conv_weight_bf16x3(wa, 32), hip.pack_conv_weight_bf16x3(wb, 32)
    else:
        w1, w2 = hip.pack_conv_weight(wa, dtype, 32), hip.pack_conv_weight(wb, dtype, 32)
    b1 = torch.zeros(C, device=dev)
    b2 = torch.zeros(C, device=dev)
    for _ in range(2):
        hip.hifigan_resunit(rb, rate, x, y, w1, b1, w2, b2, C, k, d, 0.1, dtype, **kw)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        hip.hifigan_resunit(rb, rate, x, y, w1, b1, w2, b2, C, k, d, 0.1, dtype, **kw)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    flops = 4.0 * C * C * k * rows
    byts = 2.0 * rows * C * x.element_size()
    form = f"  form {hip.resunit_variant(rb, rate, x, y, w1, b1, w2, b2, C, k, d, 0.1, dtype, **kw)}" if "variant" in kw else ""
    print(f"C={C:4d} k={k:2d} d={d} rows={rows:9d}  {ms:7.3f} ms  {flops / ms / 1e9:7.1f} TFLOP/s  {byts / ms / 1e6:7.1f} GB/s{form}")
    return ms


def run_block(C, k, rate, iters, B=64, T=768, dils=(1, 3, 5), dt=hip.F16):
    """Fused ResBlock launch against the three per-unit launches."""
    dev = torch.device("cuda:0")
    rb = hip.RaggedBatch([T] * B, dev)
    rows = B * T * rate
    g = torch.Generator(device="cpu").manual_seed(0)
    x = (torch.randn(rows, C, generator=g) * 0.5).to(dev).to(hip.torch_dtype(dt))
    bufs = [torch.empty_like(x), torch.empty_like(x)]
    units = []
    invs = []
    for d in dils:
        wa, wb = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev), (torch.randn(C, C, k, generator=g) * 0.3 / (C * k) ** 0.5).to(dev)
        if dt == hip.F32S:
            (w1, i1), (w2, i2) = hip.pack_conv_weight_split(wa, 32), hip.pack_conv_weight_split(wb, 32)
            invs.append((i1, i2))
        elif dt in hip.EMUL:
            w1, w2 = hip.pack_conv_weight_bf16x3(wa, 32), hip.pack_conv_weight_bf16x3(wb, 32)
        else:
            w1, w2 = hip.pack_conv_weight(wa, dt, 32), hip.pack_conv_weight(wb, dt, 32)
        units.append((w1, torch.zeros(C, device=dev), w2, torch.zeros(C, device=dev), d))

    def fused():
        hip.hifigan_resblock(rb, rate, x, bufs[0], units, C, k, 0.1, dt, ws=invs or None)

    def unfused():
        cur = x
        for i, (w1, b1, w2, b2, d) in enumerate(units):
            hip.hifigan_resunit(rb, rate, cur, bufs[i & 1], w1, b1, w2, b2, C, k, d, 0.1, dt, ws=invs[i] if invs else None)
            cur = bufs[i & 1]

    res = []
    for fn in (fused, unfused):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) / iters)
    flops = 4.0 * C * C * k * rows * len(dils)
    byts = 2.0 * rows * C * (2 if dt == hip.F16 else 4)      # (F32S: f32 tensors)
    print(f"ResBlock C={C:4d} k={k:2d} rows={rows:9d}: fused {res[0]:7.3f} ms ({flops / res[0] / 1e9:7.1f} TFLOP/s, {byts / res[0] / 1e6:7.1f} GB/s "
          f"of x-in + y-out)   3 unit launches {res[1]:7.3f} ms   speed-up {res[1] / res[0]:.2f}x")
    return res


# Roofs of the --single table: HBM as a float4 copy measures it; the matrix pipe at its nominal f32 / f16 rates, the emulated arithmetic at the sustained
# v_mfma_f32_16x16x32_bf16 rate on random operands (csrc/resunit_emul16_impl.h) over its seven / six MFMAs per product
HBM_GBS = 6290.0
PIPE_TFLOPS = {hip.F32: 157.3, hip.F16: 2516.0, hip.F32E: 1798.0 / 7, hip.F32E6: 1798.0 / 6}
V3_SHAPES = [(C, k, d) for C in (128, 64, 32) for k, ds in ((3, (1, 2)), (5, (2, 6)), (7, (3, 12))) for d in ds]
V3_RATES = {128: 8, 64: 64, 32: 256}       # HiFi-GAN V3 22.05 kHz stage rates (upsample scales 8, 8, 4)


def run_single(C, k, d, rate, iters, rounds=5, B=64, T=768, dtype=hip.F16):
    """Single-conv unit (w2 = None) and the two-conv unit of the same (C, k, d, rows, dtype): `rounds` alternating timings of `iters` launches each.
    Prints the medians, the two-conv unit's own spread (max - min over its rounds), algorithmic TFLOP/s (2 C^2 k rows) and GB/s (2 rows C sizeof) of the
    single-conv unit and its share of the roof that binds."""
    dev = torch.device("cuda:0")
    rb = hip.RaggedBatch([T] * B, dev)
    rows = B * T * rate
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(rows, C, generator=g).to(dev).to(hip.torch_dtype(dtype))
    y = torch.empty_like(x)
    wa, wb = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev), (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev)
    kw = {}
    if dtype in hip.EMUL:
        w1, w2 = hip.pack_unit_weight_bf16x3_k32(wa), hip.pack_unit_weight_bf16x3_k32(wb)
        kw["w_layout"] = 1
    else:
        w1, w2 = hip.pack_conv_weight(wa, dtype, 32), hip.pack_conv_weight(wb, dtype, 32)
    b1, b2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    forms = {"two": lambda: hip.hifigan_resunit(rb, rate, x, y, w1, b1, w2, b2, C, k, d, 0.1, dtype, **kw),
             "one": lambda: hip.hifigan_resunit(rb, rate, x, y, w1, b1, None, None, C, k, d, 0.1, dtype, **kw)}
    ms = {"two": [], "one": []}
    try:
        forms["two"]()
    except hip._abi.JattsHipError:      # no two-conv tile for this window (exact f32, C = 128, (k - 1) dil = 72): nothing to compare with
        del forms["two"], ms["two"]
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / iters)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    spread = max(ms["two"]) - min(ms["two"]) if "two" in ms else 0.0
    tf = 2.0 * C * C * k * rows / med["one"] / 1e9
    gbs = 2.0 * rows * C * x.element_size() / med["one"] / 1e6
    share = {"matrix": tf / PIPE_TFLOPS[dtype], "HBM": gbs / HBM_GBS}
    roof = max(share, key=share.get)
    med.setdefault("two", float("nan"))    # (refused)
    verdict = "SLOWER" if med["one"] > med["two"] + spread else "ok"
    print(f"C={C:4d} k={k:2d} d={d:2d} rows={rows:9d}  single {med['one']:7.3f} ms  two-conv {med['two']:7.3f} ms (spread {spread:.3f})  "
          f"{tf:7.1f} TFLOP/s  {gbs:7.1f} GB/s  {share[roof]:.2f} of the {roof} roof  {verdict}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, default=128)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--dil", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="f16", choices=["f16", "f32", "split", "emul", "emul6"])
    ap.add_argument("--resblock", action="store_true", help="fused ResBlock launches vs per-unit launches (f16)")
    ap.add_argument("--layout", type=int, default=1, choices=[0, 1], help="emulated units: 1 = v_mfma_f32_16x16x32_bf16 kernels (product), 0 = 32x32x16")
    ap.add_argument("--variant", type=int, default=0, choices=[0, 1, 2], help="emulated units, layout 1: 0 = the library's form, 1 = windowed, 2 = sliding")
    ap.add_argument("--variants", action="store_true", help="emulated units, layout 1: time the windowed and the sliding form of every shape")
    ap.add_argument("--single", action="store_true", help="single-conv unit (w2 = None) vs the two-conv unit at the HiFi-GAN V3 shapes (f32 / emul / emul6 / f16)")
    a = ap.parse_args()
    rates = {256: 8, 128: 64, 64: 128, 32: 256}  # HiFi-GAN v1 22.05 kHz stage rates
    dt = {"f16": hip.F16, "f32": hip.F32, "split": hip.F32S, "emul": hip.F32E, "emul6": hip.F32E6}[a.dtype]
    LAYOUT[0] = a.layout
    if a.single:
        if dt == hip.F32S:
            ap.error("--single: the split arithmetic has no single-conv unit")
        tot = {"one": 0.0, "two": 0.0}
        for C, k, d in V3_SHAPES:
            med = run_single(C, k, d, V3_RATES[C], a.iters, B=a.batch, dtype=dt)
            tot = {n: tot[n] + med[n] for n in tot}       # (two-conv: nan once a shape was refused)
        print(f"sum over the 18 units of one V3 generator pass: single {tot['one']:.2f} ms, two-conv {tot['two']:.2f} ms")
        return
    if a.resblock:
        for C in ((32, 64, 128) if dt == hip.F16 else (32, 64)):
            for k in ((3, 7) if dt != hip.F32 else (3,)):
                if dt in (hip.F32S,) + hip.EMUL and (C, k) == (64, 7):
                    continue
                run_block(C, k, rates[C], a.iters, dt=dt)
        return
    variants = (1, 2) if a.variants else (a.variant,)
    shapes = [(C, k, d) for C in (256, 128, 64, 32) for k in (3, 7, 11) for d in (1, 3, 5)] if a.all else [(a.C, a.k, a.dil)]
    tot = {v: 0.0 for v in variants}
    for C, k, d in shapes:
        ms = {v: run(C, k, d, rates[C], a.iters, B=a.batch, dtype=dt, variant=v) for v in variants}
        for v in variants:
            tot[v] += ms[v]
        if len(variants) == 2:
            print(f"    sliding / windowed = {ms[2] / ms[1]:.4f}")
    if a.all:
        for v in variants:
            print(f"sum over the 36 units of one generator pass{'' if len(variants) == 1 else f' (variant {v})'}: {tot[v]:.2f} ms")


if __name__ == "__main__":
    main()
