"""Writes tests/golden/stats_kat.npz: known answers for jatts_amd.features.FeatureStatistics / standardize.

Needs the real scikit-learn (1.7.2 when this was written): one ``StandardScaler`` per case, ``partial_fit`` per recorded call, as
jatts/bin/compute_statistics.py:75-103 runs it.  Next to sklearn's float64 results the file holds the EXACT column mean and
(population) variance of the same float32 inputs, computed in rational arithmetic and stored as double-double (hi + lo), and
sklearn's own distance from them: the yardstick the GPU tests scale their bounds by.

Per case ``<c>`` in mel, energy, spkemb, hard:
  <c>_x (rows, ld) float32, <c>_calls int64 (rows of each partial_fit, in order), <c>_dim;
  <c>_mean, <c>_var, <c>_scale float64 (dim,), <c>_n: sklearn's mean_, var_, scale_, n_samples_seen_;
  <c>_exact_mean, <c>_exact_var float64 (2, dim): hi, lo;  <c>_sk_mean_err, <c>_sk_var_err float64 (dim,): |sklearn - exact|.

    python tests/golden/make_golden_stats.py
"""
import os
from fractions import Fraction

import numpy as np
import sklearn
from sklearn.preprocessing import StandardScaler

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [1, 3, 64, 65, 127, 300]


def two_doubles(fr):
    hi = float(fr)
    return hi, float(fr - Fraction(hi))


def exact_moments(col):
    xs = [Fraction(float(v)) for v in col]
    mean = sum(xs) / len(xs)
    var = sum((v - mean) ** 2 for v in xs) / len(xs)
    return mean, var


def case(out, name, x, dim, calls):
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert sum(calls) == x.shape[0]
    sc = StandardScaler()
    r = 0
    for n in calls:
        sc.partial_fit(x[r:r + n, :dim])
        r += n
    em, ev = np.zeros((2, dim)), np.zeros((2, dim))
    me, ve = np.zeros(dim), np.zeros(dim)
    for c in range(dim):
        mean, var = exact_moments(x[:, c])
        em[:, c], ev[:, c] = two_doubles(mean), two_doubles(var)
        me[c] = float(abs(Fraction(float(sc.mean_[c])) - mean))
        ve[c] = float(abs(Fraction(float(sc.var_[c])) - var))
    out.update({f"{name}_x": x, f"{name}_calls": np.asarray(calls, dtype=np.int64), f"{name}_dim": np.int64(dim),
                f"{name}_mean": sc.mean_.astype(np.float64), f"{name}_var": sc.var_.astype(np.float64),
                f"{name}_scale": sc.scale_.astype(np.float64), f"{name}_n": np.int64(sc.n_samples_seen_),
                f"{name}_exact_mean": em, f"{name}_exact_var": ev, f"{name}_sk_mean_err": me, f"{name}_sk_var_err": ve})
    rel = ve / np.where(ev[0] > 0, ev[0], 1.0)
    print(f"{name}: rows {x.shape[0]} dim {dim} calls {list(calls)}  sklearn: max |mean err| {me.max():.3g}, max rel var err {rel.max():.3g}")


def main():
    rng = np.random.default_rng(20251019)
    out = {"sklearn_version": np.str_(sklearn.__version__)}
    rows = sum(LENGTHS)

    mel = np.empty((rows, 128), dtype=np.float32)
    mel[:, :80] = rng.normal(-5.0, 1.0, size=80)[None, :] + 2.0 * rng.standard_normal((rows, 80))
    mel[:, 80:] = 1.0e4 * rng.standard_normal((rows, 48))          # garbage on purpose: the state must not see the padding
    case(out, "mel", mel, 80, LENGTHS)

    case(out, "energy", np.abs(30.0 + 12.0 * rng.standard_normal((rows, 1))) + 0.01, 1, LENGTHS)

    case(out, "spkemb", 0.2 * rng.standard_normal((5, 192)) + 0.05 * rng.standard_normal(192)[None, :], 192, [1] * 5)

    hard = np.empty((rows, 7), dtype=np.float32)
    hard[:, 0] = rng.standard_normal(rows)
    hard[:, 1] = 4.25
    hard[:, 2] = 0.0
    hard[:, 3] = 1000.0 + 1.0e-3 * rng.standard_normal(rows)       # cancellation: a plain sum of squares loses every digit
    hard[:, 4] = 1.0e-20 * (1.0 + 0.5 * rng.standard_normal(rows))
    hard[:, 5] = 1.0e15 * (1.0 + 0.5 * rng.standard_normal(rows))
    hard[:, 6] = 3.0 + 0.7 * rng.standard_normal(rows)
    case(out, "hard", hard, 7, LENGTHS)

    path = os.path.join(HERE, "stats_kat.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
