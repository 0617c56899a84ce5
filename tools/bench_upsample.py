#!/usr/bin/env python3
"""Per-launch times of the HiFi-GAN polyphase upsampling convs (jatts_conv1d, emulated 16 x 16 x 32 kernel) at the rows of the bench batch
(64 utterances x 768 frames): the four stages of the 22.05 kHz generator (8, 8, 2, 2) and of the 24 kHz one (5, 5, 4, 3), each
  * unhinted (every tap),
  * with the tap-window hint (jatts_conv_desc.tap_group_n: two real taps per phase group) on the tile the dispatcher picks,
  * with the hint on every other tile jatts_conv_desc.variant can force for that width.
HIP events around 10 back-to-back launches, 3 warm-ups, median of 5 repeats; spread = (max - min) / median of the 5.  One JSON line per measurement.
    python tools/bench_upsample.py [--dtype emul] [--rates 22k,24k] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from jatts_amd import hip  # noqa: E402

GENERATORS = {"22k": ((8, 8, 2, 2), 512), "24k": ((5, 5, 4, 3), 512)}
WARMUP, REPEATS, LAUNCHES = 3, 5, 10


def candidates(n_out):
    """The forced tiles worth timing next to the dispatcher's choice (csrc/conv1d_emul.hip: conv1d_emul16)."""
    if n_out <= 64:
        return ()              # one tile (64 n x 64 t)
    return (2, 1) if n_out % 256 == 0 else (2, 9)


def time_launch(run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / LAUNCHES)
    ms.sort()
    return ms[REPEATS // 2], (ms[-1] - ms[0]) / ms[REPEATS // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="emul", choices=["emul", "emul6"])
    ap.add_argument("--rates", default="22k,24k")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--unhinted-only", action="store_true", help="time the every-tap launches only (e.g. with JATTS_HIP_LIB naming another build)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dt = {"emul": hip.F32E, "emul6": hip.F32E6}[a.dtype]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rb = hip.RaggedBatch([a.frames] * a.batch, dev)
    lines = []
    for name in a.rates.split(","):
        scales, c = GENERATORS[name]
        rate = 1
        for i, s in enumerate(scales):
            c_in, c_out = c, c // 2
            rows, n_out = rb.total * rate, s * c_out
            wt = torch.randn(c_in, c_out, 2 * s, generator=g) / (2.0 * c_in) ** 0.5
            wc, pad = hip.convtranspose_as_conv(wt, s, s // 2 + s % 2)
            tg = hip.convtranspose_tap_groups(2 * s, s, s // 2 + s % 2)
            win = (tg[0] * c_out,) + tg[1:]
            hip.check_tap_window(wc, win)
            w = hip.pack_conv_weight_bf16x3_k32(wc.to(dev), 64)
            x = torch.randn(rows, c_in, device=dev)
            b = torch.zeros(n_out, device=dev)
            y = torch.empty(rows, n_out, device=dev)
            ref = None
            modes = [("unhinted", 0, None)]
            if not a.unhinted_only:
                modes += [("hinted", 0, win)] + [(f"hinted v{v}", v, win) for v in candidates(n_out)]
            for label, variant, tw in modes:
                def run():
                    return hip.conv1d(rb, x, w, c_in, n_out, 3, dtype=dt, w_layout=1, pad=pad, bias=b, pre_lrelu=0.1, len_mul=rate, out=y, variant=variant,
                                      tap_window=tw)
                ms, spread = time_launch(run)
                same = True if ref is None else bool(torch.equal(y, ref))
                if ref is None:
                    ref = y.clone()
                rec = dict(gen=name, stage=i, s=s, c_in=c_in, n_out=n_out, rows=rows, mode=label, ms=round(ms, 4), spread=round(spread, 4),
                           tflops_3taps=round(2.0 * c_in * n_out * 3 * rows / ms * 1e-9, 1), equal_to_unhinted=same)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            del x, y, ref
            rate, c = rate * s, c_out
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
