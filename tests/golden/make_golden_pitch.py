"""Writes tests/golden/pitch_post_kat.npz: known answers for the steps AFTER the raw F0 track (jatts_f0_continuous_log,
jatts_energy_adjust, jatts_token_average as features.Pitch chains them).

Needs a checkout of the reference (its jatts package) and scipy: supplied raw tracks are pushed through the REAL ``Dio.forward``
(jatts/modules/feature_extract/dio.py:76-159) with ``pyworld.dio`` / ``pyworld.stonemask`` patched to return the track.  The modules the
class imports but these steps never call (pyworld, h5py, typeguard, librosa, soundfile) get empty stand-ins.  The estimator itself is
NOT in this file: parity of the raw track with DIO / StoneMask is unpinned.

Per case i < n: track_i float32 (frames,), feat_length_i (-1: None), durations_i int64 (tokens,), and for each (continuous, log) in
(1,1), (1,0), (0,1), (0,0): out_i_<c><l> float64 (tokens,), frames_i_<c><l> float64: the same without the token average.

    python tests/golden/make_golden_pitch.py --reference <path to the reference checkout>
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def import_dio(reference):
    for name in ("pyworld", "h5py", "typeguard", "librosa", "soundfile"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["typeguard"].typechecked = lambda f: f
    sys.path.insert(0, reference)
    from jatts.modules.feature_extract.dio import Dio
    return Dio


def tracks():
    g = np.random.default_rng(21)

    def voiced(n, base=150.0):
        return (base + 30.0 * np.sin(np.arange(n) / 5.0) + g.normal(0.0, 2.0, n)).astype(np.float32)

    def gaps(n, holes):
        t = voiced(n)
        for a, b in holes:
            t[a:b] = 0.0
        return t

    def durs(total, tokens, zeros=()):
        cuts = np.sort(g.integers(0, total + 1, tokens - 1 - len(zeros)))
        d = np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64)
        for z in zeros:
            d = np.insert(d, z, 0)
        assert d.sum() == total
        return d

    cases = []      # (track, feat_length or None, durations)
    t = gaps(60, [(0, 7), (51, 60)])
    cases.append((t, None, durs(60, 9)))                                  # unvoiced lead and tail
    t = gaps(80, [(0, 3), (20, 29), (30, 31), (47, 66), (77, 80)])
    cases.append((t, None, durs(80, 12, zeros=(0, 5, 11))))               # interior gaps; zero-duration tokens
    t = np.zeros(40, dtype=np.float32)
    t[17] = 212.5
    cases.append((t, None, durs(40, 6)))                                  # a single voiced frame
    cases.append((np.zeros(33, dtype=np.float32), None, durs(33, 5)))      # all unvoiced
    t = gaps(50, [(10, 20), (35, 44)])
    cases.append((t, None, durs(50, 8)))                                  # voiced first and last frame
    t = gaps(70, [(0, 5), (30, 40), (64, 70)])
    t[5] = t[9] = t[12] = 180.25                                          # the first voiced value repeats later
    t[63] = t[57] = t[50] = 141.5                                         # the last voiced value occurs earlier
    cases.append((t, None, durs(70, 10)))
    t = gaps(90, [(0, 4), (40, 52), (80, 90)])
    cases.append((t, 75, durs(75, 11)))                                   # feat_length shorter than the track
    cases.append((t.copy(), 97, durs(97, 11, zeros=(3,))))                # feat_length longer: zero-padded frames
    t = gaps(1500, [(0, 100), (600, 700), (1023, 1030), (1400, 1500)])
    cases.append((t, None, durs(1500, 150)))                              # longer than one scan chunk of the kernel
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory that holds jatts/)")
    args = ap.parse_args()
    Dio = import_dio(os.path.abspath(args.reference))
    pyworld = sys.modules["pyworld"]
    out = {}
    cases = tracks()
    for i, (track, feat_length, d) in enumerate(cases):
        pyworld.dio = lambda x, fs, f0_floor, f0_ceil, frame_period, _t=track: (_t.astype(np.float64), np.arange(_t.size) * frame_period / 1000.0)
        pyworld.stonemask = lambda x, f0, timeaxis, fs: f0
        out[f"track_{i}"] = track
        out[f"feat_length_{i}"] = np.int64(-1 if feat_length is None else feat_length)
        out[f"durations_{i}"] = d
        for cont in (1, 0):
            for log in (1, 0):
                ext = Dio(fs=24000, n_fft=2048, hop_length=300, use_token_averaged_f0=True, use_continuous_f0=bool(cont), use_log_f0=bool(log),
                          reduction_factor=1)
                out[f"out_{i}_{cont}{log}"] = np.asarray(ext.forward(np.zeros(16, dtype=np.float32), 70, 400, feat_length, d), dtype=np.float64)
                ext.use_token_averaged_f0 = False
                out[f"frames_{i}_{cont}{log}"] = np.asarray(ext.forward(np.zeros(16, dtype=np.float32), 70, 400, feat_length, None), dtype=np.float64)
    out["n"] = np.int64(len(cases))
    np.savez_compressed(os.path.join(HERE, "pitch_post_kat.npz"), **out)
    print("wrote pitch_post_kat.npz:", len(cases), "cases")


if __name__ == "__main__":
    main()
