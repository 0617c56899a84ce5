"""Time one statistics update (FeatureStatistics.partial_fit, csrc/stats.hip) at the bench geometry against what a user would
otherwise write: the torch composition on the device (float64 moments + the pairwise update) and sklearn on the host (copy included).

Geometry: 64 utterances x 768 frames of log-mel, 80 live columns in a row pitch of 128, and the dim = 1 vector (energy / pitch) of
the same rows.  The three contenders alternate inside every repetition; each timing is `inner` back-to-back calls between two
device events (the host path: a host clock around a call that ends in the copy's synchronisation).  Prints a table (median and
min .. max over the repetitions) and the share of the HBM peak the new kernels reach, counting the bytes the update must read
(rows x dim x 4; the state and the partial sums are noise).  Needs a GPU; numbers from anything else are not measurements.

    python tools/bench_stats.py [--reps 15] [--inner 40] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes / s, MI355X specification


def torch_update(state, x, dim):
    """The device composition a user would write: float64 batch moments and the Chan update of (n, mean, M2) tensors."""
    n_a, mean_a, m2_a = state
    xd = x[:, :dim].double() if x.dim() == 2 else x.double().unsqueeze(1)
    n_b = xd.shape[0]
    mean_b = xd.sum(0) / n_b
    m2_b = ((xd - mean_b) ** 2).sum(0)
    n = n_a + n_b
    delta = mean_b - mean_a
    return n, mean_a + delta * (n_b / n), m2_a + m2_b + delta * delta * (n_a * n_b / n)


def device_time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--inner", type=int, default=40)
    p.add_argument("--json", type=str, default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats needs a GPU: nothing is measured without one")
    from jatts_amd.features import FeatureStatistics
    try:
        from sklearn.preprocessing import StandardScaler
    except ImportError:
        StandardScaler = None
    dev = torch.device("cuda")
    rows = 64 * 768
    g = torch.Generator().manual_seed(0)
    shapes = {"mel 80 in ld 128": (torch.randn(rows, 128, generator=g) * 2 - 5, 80), "dim 1": (torch.rand(rows, generator=g) * 40 + 1, 1)}
    result = {"rows": rows, "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, (xh, dim) in shapes.items():
        x = xh.to(dev)
        acc = FeatureStatistics(dim, dev)
        tstate = [(0.0, torch.zeros(dim, dtype=torch.float64, device=dev), torch.zeros(dim, dtype=torch.float64, device=dev))]
        sk = StandardScaler() if StandardScaler is not None else None

        def ours():
            acc.partial_fit(x)

        def composed():
            tstate[0] = torch_update(tstate[0], x, dim)

        def host():
            t0 = time.perf_counter()
            a = x.cpu().numpy()
            sk.partial_fit(a[:, :dim] if a.ndim == 2 else a.reshape(-1, 1))
            return time.perf_counter() - t0

        for _ in range(3):                     # warm every contender at this shape
            ours(), composed()
            if sk is not None:
                host()
        torch.cuda.synchronize()
        t = {"partial_fit": [], "torch float64 composition": [], "sklearn on the host (copy included)": []}
        for _ in range(args.reps):
            t["partial_fit"].append(device_time(ours, args.inner))
            t["torch float64 composition"].append(device_time(composed, args.inner))
            if sk is not None:
                t["sklearn on the host (copy included)"].append(statistics.mean(host() for _ in range(2)))
        need = rows * dim * 4
        rec = {}
        print(f"\n{name}: {rows} rows, {need / 1e6:.2f} MB to read per update")
        for k, v in t.items():
            if not v:
                print(f"  {k:40s} not measured (sklearn missing)")
                continue
            med = statistics.median(v)
            rec[k] = {"median_us": med * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6}
            print(f"  {k:40s} median {med * 1e6:9.1f} us   min {min(v) * 1e6:9.1f}   max {max(v) * 1e6:9.1f}")
        med = rec["partial_fit"]["median_us"] * 1e-6
        rec["partial_fit_bytes_per_s"] = need / med
        rec["partial_fit_share_of_hbm_peak"] = need / med / HBM_PEAK
        print(f"  partial_fit: {need / med / 1e12:.3f} TB/s = {100 * need / med / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak "
              f"(memory-bound: {need / HBM_PEAK * 1e6:.2f} us at peak; two launches per update)")
        # the two device paths agree on what they computed
        mean, var, _, _ = acc.finalize()
        n_t, mean_t, m2_t = tstate[0]
        rec["max_rel_mean_diff_vs_torch"] = float(np.max(np.abs(mean - mean_t.cpu().numpy()) / np.abs(mean)))
        rec["max_rel_var_diff_vs_torch"] = float(np.max(np.abs(var - (m2_t / n_t).cpu().numpy()) / var))
        print(f"  agreement with the torch composition: mean {rec['max_rel_mean_diff_vs_torch']:.2e}, var {rec['max_rel_var_diff_vs_torch']:.2e} (relative)")
        result["shapes"][name] = rec
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
