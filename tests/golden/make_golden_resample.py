"""Writes tests/golden/resample_kat.npz: known-answer data for the sample-rate converter of jatts_amd.features
(tests/test_resample_cpu.py, tests/test_resample_gpu.py).

Run on a CPU host (python tests/golden/make_golden_resample.py); the suite runs it only to check that it reproduces the file, byte
for byte (the archive is written with fixed member dates).

librosa, soxr and resampy are not installed where this project is built, so parity with librosa.load(sr=...) (soxr_hq) stays
UNPINNED.  What is pinned is the polyphase arithmetic: the answers come from the real scipy.signal.resample_poly in float64, called
with explicit taps.  The taps are scipy's own too -- up * scipy.signal.firwin(2 * half_len + 1, rolloff / max(up, down),
window=("kaiser", beta)), rounded to float32 once -- so nothing here imports jatts_amd.

Per case (a ratio and a filter design) and per input (seeded noise at amplitude 0.1; one chirp over the whole band):
  y64  resample_poly(x, up, down, window=h / up) in float64 on the float32-rounded taps h (resample_poly multiplies by up itself)
  S    resample_poly(|x|, up, down, window=|h| / up): the per-output sum |h| |x|, what every rounding-error bound scales with
and per case E32 = max over both inputs and all outputs of |y32 - y64| / S for scipy's own float32 arithmetic: scipy.signal.upfirdn,
the routine resample_poly runs, on float32 input with the float32 taps placed exactly as resample_poly places them (resample_poly
itself would form up * (h / up) in float32, which is not h when up is no power of two; the float64 form of the same call is checked
against resample_poly below).
"""
import io
import json
import os
import zipfile

import numpy as np
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
KAISER_BEST = dict(zeros=64, rolloff=0.9475937167399596, beta=14.769656459379492)      # the published "kaiser_best" constants
SCIPY_DEFAULT = dict(zeros=10, rolloff=1.0, beta=5.0)                                    # resample_poly's own design
CASES = [
    ("48k_24k", 48000, 24000, KAISER_BEST),
    ("48k_16k", 48000, 16000, KAISER_BEST),
    ("24k_16k", 24000, 16000, KAISER_BEST),
    ("44k1_24k", 44100, 24000, KAISER_BEST),
    ("22k05_24k", 22050, 24000, KAISER_BEST),
    ("24k_44k1", 24000, 44100, KAISER_BEST),
    ("24k_48k", 24000, 48000, KAISER_BEST),
    ("44k1_24k_scipy", 44100, 24000, SCIPY_DEFAULT),
]
N_NOISE, N_CHIRP = 2001, 1000


def inputs():
    rng = np.random.default_rng(20251019)
    noise = (0.1 * rng.standard_normal(N_NOISE)).astype(np.float32)
    t = np.arange(N_CHIRP, dtype=np.float64)
    chirp = (0.5 * np.sin(2.0 * np.pi * (0.25 / N_CHIRP) * t * t)).astype(np.float32)     # 0 -> 0.5 cycles per sample
    return {"noise": noise, "chirp": chirp}


def taps32(sr_in, sr_out, zeros, rolloff, beta):
    g = np.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    m = max(up, down)
    h = up * signal.firwin(2 * zeros * m + 1, rolloff / m, window=("kaiser", beta))
    return int(up), int(down), h.astype(np.float32)


def upfirdn_as_resample_poly(x, h, up, down):
    """resample_poly's own placement of the taps (scipy/signal/_signaltools.py), with h used as it is (not up * (h / up))."""
    n_in, half_len = x.shape[0], (h.size - 1) // 2
    n_out = -(-n_in * up // down)
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    n_post_pad = 0
    while ((n_in - 1) * up + h.size + n_pre_pad + n_post_pad - 1) // down + 1 < n_out + n_pre_remove:      # upfirdn's output length
        n_post_pad += 1
    hp = np.concatenate((np.zeros(n_pre_pad, h.dtype), h, np.zeros(n_post_pad, h.dtype)))
    y = signal.upfirdn(hp, x, up, down)
    return y[n_pre_remove:n_pre_remove + n_out]


def build():
    """-> dict of arrays, in the order they are written"""
    out = {}
    xs = inputs()
    for k, v in xs.items():
        out[f"x_{k}"] = v
    meta = []
    for name, sr_in, sr_out, design in CASES:
        up, down, h = taps32(sr_in, sr_out, **design)
        h64 = h.astype(np.float64)
        e32 = 0.0
        for k, x in xs.items():
            x64 = x.astype(np.float64)
            y64 = signal.resample_poly(x64, up, down, window=h64 / up)
            s = signal.resample_poly(np.abs(x64), up, down, window=np.abs(h64) / up)
            assert y64.shape[0] == -(-x.shape[0] * up // down) and s.min() > 0.0
            chk = upfirdn_as_resample_poly(x64, h64, up, down)
            assert chk.shape == y64.shape and np.abs(chk - y64).max() <= 1e-14 * s.max()
            y32 = upfirdn_as_resample_poly(x, h, up, down)
            assert y32.dtype == np.float32
            e32 = max(e32, float((np.abs(y32.astype(np.float64) - y64) / s).max()))
            out[f"{name}_{k}_y64"] = y64
            out[f"{name}_{k}_S"] = s
        out[f"{name}_E32"] = np.float64(e32)
        meta.append(dict(name=name, sr_in=sr_in, sr_out=sr_out, up=up, down=down, **design))
    out["cases"] = np.array(json.dumps(meta))
    return out


def write_npz(path, arrays):
    """An .npz numpy.load reads, with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main(path=os.path.join(HERE, "resample_kat.npz")):
    arrays = build()
    write_npz(path, arrays)
    for k, v in arrays.items():
        if k.endswith("_E32"):
            print(f"{k}: {float(v):.3e}")
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
