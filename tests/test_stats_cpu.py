"""CPU: the host side of the stage-1 statistics (jatts_amd.features.stats_from_state / save_stats) against the sklearn fixture
tests/golden/stats_kat.npz (tests/golden/make_golden_stats.py), and the new C-ABI symbols.  No compute calls (no GPU here)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("jatts_stats_rows_per_group", "jatts_col_moments", "jatts_col_moments_merge", "jatts_standardize")
CASES = ("mel", "energy", "spkemb", "hard")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "stats_kat.npz"))


@pytest.mark.parametrize("case", CASES)
def test_stats_from_state_reproduces_sklearn(kat, case):
    """Fed the EXACT n, mean and M2 = n var of the inputs, the finalisation gives sklearn's var_ to sklearn's own distance from the exact
    value (plus the roundings of n var / n) and sklearn's scale_ to half of that relative distance -- including the constant-feature rule."""
    from jatts_amd.features import stats_from_state
    n = float(kat[f"{case}_n"])
    em, ev = kat[f"{case}_exact_mean"][0], kat[f"{case}_exact_var"][0]
    mean, var, scale = stats_from_state(np.full(em.shape, n), em, ev * n)
    assert mean.dtype == var.dtype == scale.dtype == np.float64
    sk_var, sk_scale = kat[f"{case}_var"], kat[f"{case}_scale"]
    tol_var = kat[f"{case}_sk_var_err"] + 4 * EPS * ev
    assert np.all(np.abs(var - sk_var) <= tol_var), np.abs(var - sk_var) / np.maximum(tol_var, 1e-300)
    assert np.all(np.abs(mean - kat[f"{case}_mean"]) <= kat[f"{case}_sk_mean_err"] + EPS * np.abs(em))
    constant = sk_var == 0
    assert np.array_equal(scale[constant], np.ones(int(constant.sum()))) and np.array_equal(sk_scale[constant], scale[constant])
    live = ~constant
    rel = tol_var[live] / ev[live] + 4 * EPS
    assert np.all(np.abs(scale[live] - sk_scale[live]) <= rel * sk_scale[live])


def test_constant_zero_and_tiny_columns(kat):
    from jatts_amd.features import stats_from_state
    n = float(kat["hard_n"])
    em, ev = kat["hard_exact_mean"][0], kat["hard_exact_var"][0]
    _, var, scale = stats_from_state(np.full(7, n), em, ev * n)
    assert var[1] == 0.0 and scale[1] == 1.0 and em[1] == 4.25                 # constant: scale 1, not 0
    assert var[2] == 0.0 and scale[2] == 1.0 and em[2] == 0.0                  # all zeros
    assert 0.0 < scale[4] < 1e-19 and scale[4] == np.sqrt(var[4])              # values of order 1e-20 are NOT constant
    assert scale[5] > 1e14
    # a variance at the two-pass algorithm's error level counts as constant (sklearn's _is_constant_feature)
    _, _, s = stats_from_state([100.0, 100.0], [1000.0, 1000.0], [100.0 * (100 * 1000.0 * EPS) ** 2, 100.0 * 1e-6])
    assert s[0] == 1.0 and s[1] == pytest.approx(1e-3)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            stats_from_state([5.0, 5.0], [0.0, bad], [1.0, 1.0])
        with pytest.raises(ValueError):
            stats_from_state([5.0, 5.0], [0.0, 0.0], [1.0, bad])
    with pytest.raises(ValueError):
        stats_from_state([0.0], [0.0], [0.0])


def test_save_round_trips_through_read_stats(tmp_path, kat):
    from jatts_amd.bin.tts_decode import read_stats
    from jatts_amd.features import save_stats
    path = str(tmp_path / "stats.npz")
    save_stats(path, "mel", kat["mel_mean"], kat["mel_scale"])
    save_stats(path, "energy", kat["energy_mean"], kat["energy_scale"])          # the second feature keeps the first
    for feat in ("mel", "energy"):
        st = read_stats(path, feat)
        assert st["mean"].dtype == st["scale"].dtype == np.float32
        assert np.array_equal(st["mean"], kat[f"{feat}_mean"].astype(np.float32))
        assert np.array_equal(st["scale"], kat[f"{feat}_scale"].astype(np.float32))
    save_stats(path, "mel", kat["mel_mean"] + 1.0, kat["mel_scale"])              # an update replaces, and keeps the other
    assert np.array_equal(read_stats(path, "mel")["mean"], (kat["mel_mean"] + 1.0).astype(np.float32))
    assert np.array_equal(read_stats(path, "energy")["mean"], kat["energy_mean"].astype(np.float32))
    with np.load(path) as z:
        assert sorted(z.files) == ["energy_mean", "energy_scale", "mel_mean", "mel_scale"]
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="needs h5py"):
            save_stats(str(tmp_path / "stats.h5"), "mel", kat["mel_mean"], kat["mel_scale"])
    else:
        save_stats(str(tmp_path / "stats.h5"), "mel", kat["mel_mean"], kat["mel_scale"])
        assert np.array_equal(read_stats(str(tmp_path / "stats.h5"), "mel")["scale"], kat["mel_scale"].astype(np.float32))


def test_new_symbols_in_header_mirror_and_library(lib):
    from jatts_amd import _abi, features
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    declared = set(re.findall(r"\b(jatts_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _abi.PROTOTYPES and hasattr(lib, name), name
    assert int(re.search(r"#define JATTS_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _abi.ABI_VERSION == lib.jatts_abi_version()
    r = int(re.search(r"#define JATTS_STATS_ROWS_PER_GROUP (\d+)", hdr).group(1))
    assert r == lib.jatts_stats_rows_per_group() == _abi.STATS_ROWS_PER_GROUP == features.STATS_ROWS_PER_GROUP


def test_fixture_holds_what_the_issue_lists(kat):
    assert str(kat["sklearn_version"]).split(".")[0].isdigit()
    assert list(kat["mel_calls"]) == [1, 3, 64, 65, 127, 300] == list(kat["energy_calls"])
    assert kat["mel_x"].shape == (560, 128) and int(kat["mel_dim"]) == 80 and kat["mel_x"].dtype == np.float32
    assert float(np.abs(kat["mel_x"][:, 80:]).max()) > 100.0                      # the padding holds garbage on purpose
    assert kat["energy_x"].shape == (560, 1) and float(kat["energy_x"].min()) > 0
    assert kat["spkemb_x"].shape == (5, 192) and list(kat["spkemb_calls"]) == [1] * 5
    assert kat["hard_x"].shape[1] == 7 and kat["hard_scale"][1] == 1.0 and kat["hard_var"][1] == 0.0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "stats_kat.npz")) < 512 * 1024
