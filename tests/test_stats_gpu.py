"""GPU: jatts_amd.features.FeatureStatistics / standardize / bin.compute_statistics (csrc/stats.hip) against the sklearn fixture
tests/golden/stats_kat.npz (real sklearn StandardScaler.partial_fit, plus the exact moments of the same inputs) and against exact
moments computed here.

Accuracy rule: per column |mean - exact| and |var - exact| may be at most 2 x sklearn's own distance from the exact value (recorded in
the fixture), or, where that is smaller (it can be exactly 0), the worst-case bound of an ordered float64 sum:
    n 2^-53 max |x|            for the mean,
    4 n 2^-53 max (x - mean)^2 for the variance.
Every test prints its largest error / bound ratio."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
CASES = ("mel", "energy", "spkemb", "hard")


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "stats_kat.npz"))


def run_calls(cuda, x_dev, dim, calls):
    from jatts_amd.features import FeatureStatistics
    acc = FeatureStatistics(dim, cuda)
    r = 0
    for n in calls:
        acc.partial_fit(x_dev[r:r + int(n)])
        r += int(n)
    return acc


def bound_ratios(mean, var, x64, exact_mean, exact_var, sk_mean_err=0.0, sk_var_err=0.0):
    """-> (worst mean ratio, worst var ratio) of error / max(2 x sklearn's error, floor); exact_*: (hi, lo) double-double rows."""
    n = x64.shape[0]
    mean_err = np.abs((mean - exact_mean[0]) - exact_mean[1])
    var_err = np.abs((var - exact_var[0]) - exact_var[1])
    bm = np.maximum(2.0 * np.asarray(sk_mean_err), n * U * np.abs(x64).max(axis=0))
    bv = np.maximum(2.0 * np.asarray(sk_var_err), 4.0 * n * U * ((x64 - exact_mean[0]) ** 2).max(axis=0))

    def ratio(err, bound):
        out = np.zeros_like(err)
        nz = bound > 0
        out[nz] = err[nz] / bound[nz]
        out[~nz & (err > 0)] = np.inf          # a zero bound (constant column) admits only a zero error
        return float(out.max())
    return ratio(mean_err, bm), ratio(var_err, bv)


@pytest.mark.parametrize("case", CASES)
def test_accuracy_against_sklearn_and_exact(cuda, lib, kat, case):
    dim = int(kat[f"{case}_dim"])
    x = kat[f"{case}_x"]
    acc = run_calls(cuda, torch.from_numpy(x).to(cuda), dim, kat[f"{case}_calls"])
    mean, var, scale, n = acc.finalize()
    assert mean.dtype == var.dtype == scale.dtype == np.float64 and mean.shape == (dim,)
    assert n == int(kat[f"{case}_n"]) == acc.n_samples_seen_
    rm, rv = bound_ratios(mean, var, x[:, :dim].astype(np.float64), kat[f"{case}_exact_mean"], kat[f"{case}_exact_var"],
                          kat[f"{case}_sk_mean_err"], kat[f"{case}_sk_var_err"])
    print(f"\n[stats accuracy] {case}: error / bound  mean {rm:.3g}  var {rv:.3g}")
    assert rm <= 1.0 and rv <= 1.0
    # what the stats file stores
    eq = []
    for ours, want in ((mean, kat[f"{case}_mean"]), (scale, kat[f"{case}_scale"])):
        a, b = ours.astype(np.float32), want.astype(np.float32)
        eq.append(int((a == b).sum()))
        assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)), case
    print(f"[stats f32] {case}: bit-equal to sklearn's float32 casts: mean {eq[0]} / {dim}, scale {eq[1]} / {dim}")
    if case == "hard":
        assert var[1] == 0.0 and scale[1] == 1.0 and mean[1] == 4.25 and var[2] == 0.0 and scale[2] == 1.0 and mean[2] == 0.0


# ---- group boundaries: data on a 2^-8 grid, so that the exact moments are integer arithmetic
def _grid_data():
    from jatts_amd.features import STATS_ROWS_PER_GROUP as R
    rng = np.random.default_rng(7)
    k = np.rint(256.0 * (rng.normal(-5.0, 1.0, size=128)[None, :] + 2.0 * rng.standard_normal((3 * R + 5, 128)))).astype(np.int64)
    return k


@pytest.fixture(scope="module")
def grid():
    return _grid_data()


def exact_grid_moments(k):
    """k: int64 (n, dim), x = k / 256 -> double-double (2, dim) exact mean and population variance."""
    n = k.shape[0]
    em, ev = np.zeros((2, k.shape[1])), np.zeros((2, k.shape[1]))
    for c in range(k.shape[1]):
        s, s2 = int(k[:, c].sum()), int((k[:, c] * k[:, c]).sum())
        for out, fr in ((em, Fraction(s, 256 * n)), (ev, Fraction(n * s2 - s * s, 65536 * n * n))):
            hi = float(fr)
            out[:, c] = hi, float(fr - Fraction(hi))
    return em, ev


def _rows_options():
    from jatts_amd.features import STATS_ROWS_PER_GROUP as R
    return [1, R - 1, R, R + 1, 3 * R + 5]


@pytest.mark.parametrize("dim,ld", [(1, 1), (3, 3), (80, 128), (100, 100)])
@pytest.mark.parametrize("rows_i", range(5))
def test_group_boundaries(cuda, lib, grid, rows_i, dim, ld):
    from jatts_amd.features import STATS_ROWS_PER_GROUP as R
    rows = _rows_options()[rows_i]
    k = grid[:rows, :ld]
    x = (k.astype(np.float64) / 256.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 256.0, k.astype(np.float64))         # the grid is exact in float32
    em, ev = exact_grid_moments(k[:, :dim])
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    splits = [[rows]] + ([[R - 1, rows - (R - 1)]] if rows > R - 1 else [])
    for calls in splits:
        mean, var, _, n = run_calls(cuda, xd, dim, calls).finalize()
        assert n == rows
        rm, rv = bound_ratios(mean, var, x[:, :dim].astype(np.float64), em, ev)
        print(f"\n[stats groups] rows {rows} dim {dim} ld {ld} calls {calls}: error / floor  mean {rm:.3g}  var {rv:.3g}")
        assert rm <= 1.0 and rv <= 1.0, (rows, dim, calls)


def test_state_does_not_depend_on_the_row_pitch(cuda, lib, grid):
    """The same rows and dim through the 16-byte loads (ld % 4 == 0) and the scalar ones (odd ld, or a base that is not 16-byte aligned):
    identical bits -- the result is a function of the calls, their rows and dim only."""
    from jatts_amd.features import STATS_ROWS_PER_GROUP as R
    rows, dim = R + 7, 3
    x = (grid[:rows, :8].astype(np.float64) / 256.0).astype(np.float32)
    states = []
    for ld in (3, 4, 5, 8):
        states.append(run_calls(cuda, torch.from_numpy(np.ascontiguousarray(x[:, :ld])).to(cuda), dim, [R - 1, 8]).state.clone())
    flat = torch.zeros(rows * 4 + 1, dtype=torch.float32, device=cuda)
    flat[1:] = torch.from_numpy(np.ascontiguousarray(x[:, :4])).to(cuda).reshape(-1)
    states.append(run_calls(cuda, flat[1:].view(rows, 4), dim, [R - 1, 8]).state.clone())
    for s in states[1:]:
        assert torch.equal(s, states[0])


def test_same_calls_give_the_same_bits(cuda, lib, kat):
    x = torch.from_numpy(kat["mel_x"]).to(cuda)
    big = torch.from_numpy(np.tile(kat["mel_x"], (8, 1))).to(cuda)           # 4480 rows: five groups
    a = run_calls(cuda, x, 80, kat["mel_calls"]).partial_fit(big)
    b = run_calls(cuda, x, 80, kat["mel_calls"]).partial_fit(big)
    assert a.state.dtype == torch.float64 and a.state.shape == (3, 80)
    assert torch.equal(a.state, b.state)


def test_merge_of_two_halves(cuda, lib, kat):
    x = torch.from_numpy(kat["mel_x"]).to(cuda)
    calls = [int(v) for v in kat["mel_calls"]]
    first = sum(calls[:4])
    a = run_calls(cuda, x[:first], 80, calls[:4])
    b = run_calls(cuda, x[first:], 80, calls[4:])
    b_state = b.state.clone()
    mean, var, _, n = a.merge(b).finalize()
    assert n == 560 and torch.equal(b.state, b_state)
    rm, rv = bound_ratios(mean, var, kat["mel_x"][:, :80].astype(np.float64), kat["mel_exact_mean"], kat["mel_exact_var"],
                          kat["mel_sk_mean_err"], kat["mel_sk_var_err"])
    print(f"\n[stats merge] mel, calls 0-3 | 4-5: error / bound  mean {rm:.3g}  var {rv:.3g}")
    assert rm <= 1.0 and rv <= 1.0
    from jatts_amd.features import FeatureStatistics
    empty = FeatureStatistics(80, cuda)
    assert torch.equal(empty.merge(b).state, b_state)                         # into an empty accumulator: a copy
    assert torch.equal(b.merge(FeatureStatistics(80, cuda)).state, b_state)   # an empty one changes nothing


def test_partial_fit_does_not_synchronise(cuda, lib, kat):
    from jatts_amd import hip
    from jatts_amd.features import FeatureStatistics
    x = torch.from_numpy(kat["mel_x"]).to(cuda)
    e = torch.from_numpy(kat["energy_x"]).to(cuda)
    rb = hip.RaggedBatch([int(v) for v in kat["mel_calls"]], cuda)
    acc, acc_r, acc_e, other = (FeatureStatistics(d, cuda) for d in (80, 80, 1, 80))
    other.partial_fit(x[:10])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = 0
        for n in kat["mel_calls"]:
            acc.partial_fit(x[r:r + int(n)])
            acc_e.partial_fit(e[r:r + int(n)].reshape(-1))                     # (rows,) with dim 1
            r += int(n)
        acc.partial_fit(x[:0])                                                 # rows = 0: a no-op
        acc_r.partial_fit_ragged(rb, x)
        acc_r.merge(other)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert acc.finalize()[3] == 560 and acc_e.finalize()[3] == 560 and acc_r.finalize()[3] == 570
    assert torch.equal(run_calls(cuda, x, 80, kat["mel_calls"]).state, acc.state)
    assert torch.equal(run_calls(cuda, x, 80, [560]).merge(other).state, acc_r.state)   # the packed rows of a batch are ONE call


def test_non_finite_values_are_refused_at_finalize(cuda, lib, kat):
    from jatts_amd.features import FeatureStatistics
    x = torch.from_numpy(kat["hard_x"]).to(cuda).clone()
    x[17, 3] = float("nan")
    acc = FeatureStatistics(7, cuda).partial_fit(x)
    with pytest.raises(ValueError):
        acc.finalize()
    with pytest.raises(ValueError):
        FeatureStatistics(7, cuda).finalize()                                   # no sample


@pytest.mark.parametrize("case", ("mel", "hard"))
def test_standardize_is_numpy_float32_bit_for_bit(cuda, lib, kat, case):
    from jatts_amd.features import standardize
    dim = int(kat[f"{case}_dim"])
    x = kat[f"{case}_x"]
    m32, s32 = kat[f"{case}_mean"].astype(np.float32), kat[f"{case}_scale"].astype(np.float32)
    want = (x[:, :dim] - m32) / s32
    assert want.dtype == np.float32
    y = standardize(torch.from_numpy(x).to(cuda), m32, s32)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == x.shape
    got = y.cpu().numpy()
    assert np.array_equal(got[:, :dim].view(np.int32), want.view(np.int32))
    assert not np.any(got[:, dim:].view(np.int32))                              # padding columns: exactly +0
    if case == "hard":
        assert s32[1] == 1.0 and s32[2] == 1.0 and not np.any(got[:, 1:3])
    else:
        y2 = standardize(torch.from_numpy(x).to(cuda), torch.from_numpy(m32).to(cuda), torch.from_numpy(s32).to(cuda), dim=77)
        assert np.array_equal(y2.cpu().numpy()[:, :77].view(np.int32), want[:, :77].view(np.int32)) and not np.any(y2.cpu().numpy()[:, 77:])


def test_cli_writes_the_accumulators_stats(cuda, lib, kat, tmp_path):
    from jatts_amd.bin.tts_decode import read_stats
    rng = np.random.default_rng(3)
    lens, paths = [37, 64, 129], []
    for i, n in enumerate(lens):
        p = str(tmp_path / f"utt{i}.npz")
        np.savez(p, wave=rng.standard_normal(256 * n).astype(np.float32), mel=kat["mel_x"][100 * i:100 * i + n, :80],
                 energy=kat["energy_x"][100 * i:100 * i + n, 0], spkemb=kat["spkemb_x"][i])
        paths.append(p)
    csv_path, out = str(tmp_path / "train.csv"), str(tmp_path / "stats.npz")
    with open(csv_path, "w") as f:
        f.write("sample_id,feat_path\n" + "".join(f"utt{i},{p}\n" for i, p in enumerate(paths)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "jatts_amd.bin.compute_statistics", "--csv", csv_path, "--out", out, "--verbose", "0"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        assert sorted(z.files) == sorted(f"{k}_{s}" for k in ("mel", "energy", "spkemb") for s in ("mean", "scale"))       # no wave
    for feat, dim, rows in (("mel", 80, lambda i, n: kat["mel_x"][100 * i:100 * i + n, :80]),
                            ("energy", 1, lambda i, n: kat["energy_x"][100 * i:100 * i + n, :1]),
                            ("spkemb", 192, lambda i, n: kat["spkemb_x"][i:i + 1])):
        from jatts_amd.features import FeatureStatistics
        acc = FeatureStatistics(dim, cuda)
        for i, n in enumerate(lens):
            acc.partial_fit(torch.from_numpy(np.ascontiguousarray(rows(i, n))).to(cuda))
        mean, _, scale, _ = acc.finalize()
        st = read_stats(out, feat)
        assert np.array_equal(st["mean"], mean.astype(np.float32)) and np.array_equal(st["scale"], scale.astype(np.float32)), feat


def test_cpu_tensors_raise(cuda, lib):
    from jatts_amd._abi import JattsHipError
    from jatts_amd.features import FeatureStatistics, standardize
    with pytest.raises(JattsHipError):
        FeatureStatistics(80, "cpu")
    with pytest.raises(JattsHipError):
        FeatureStatistics(80, cuda).partial_fit(torch.zeros(4, 80))
    with pytest.raises(JattsHipError):
        standardize(torch.zeros(4, 80), np.zeros(80, np.float32), np.ones(80, np.float32))
    with pytest.raises(ValueError):
        FeatureStatistics(80, cuda).partial_fit(torch.zeros(4, 64, device=cuda))      # ld < dim
