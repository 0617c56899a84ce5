"""CPU: the stage-5 restatements themselves (tests/evaluate_reference.py) and the host side of jatts_amd.evaluate / jatts_amd.bin.evaluate.
The restated DTW is held to brute-force enumeration of every monotone path; the refusals raise by name before any file is touched."""
import numpy as np
import pytest

import evaluate_reference as ER


def _costs(kind, n, m, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.random((n, m)) + 0.01).astype(np.float32)
    return rng.integers(0, 3, (n, m)).astype(np.float32)


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_dtw_equals_enumeration_of_all_monotone_paths(kind):
    for n in range(1, 6):
        for m in range(1, 6):
            c = _costs(kind, n, m, 100 * n + m)
            pi, pj, total = ER.dtw(c)
            paths = ER.monotone_paths(n, m)
            sums = [sum(float(c[a, b]) for a, b in p) for p in paths]
            assert total == min(sums), (n, m)                                   # the same float64 adds in the same order: equal, not close
            want, best = ER.tie_rule_path(c)
            assert best == total and list(zip(pi.tolist(), pj.tolist())) == want, (n, m)
            assert sum(float(c[a, b]) for a, b in want) == total
            qi, qj, qt = ER.dtw_fast(c)
            assert qt == total and np.array_equal(qi, pi) and np.array_equal(qj, pj)


def test_dtw_fast_equals_double_loop_on_larger_shapes():
    for n, m, kind in ((37, 23, "random"), (23, 37, "ties"), (1, 40, "random"), (40, 1, "ties"), (64, 64, "ties")):
        c = _costs(kind, n, m, n + m)
        a, b = ER.dtw(c), ER.dtw_fast(c)
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert max(n, m) <= a[0].size <= n + m - 1


def test_dct_matrix_is_orthonormal():
    from jatts_amd.evaluate import dct_matrix
    full = dct_matrix(80, 80)
    assert np.abs(full @ full.T - np.eye(80)).max() < 1e-13
    w = dct_matrix()
    assert w.shape == (40, 80) and w.dtype == np.float64
    assert np.abs(w @ w.T - np.eye(40)).max() < 1e-13
    assert np.array_equal(w, ER.dct_matrix(80, 40)) and np.array_equal(w, full[:40])


def test_cli_refusals_raise_by_name_without_touching_a_file(tmp_path):
    from jatts_amd.bin import evaluate as cli
    missing = str(tmp_path / "does_not_exist")
    for metric, exc, word in (("asr", NotImplementedError, "nue_asr"), ("sheet", NotImplementedError, "SHEET")):
        with pytest.raises(exc, match=word):
            cli.main(["--wavdir", missing, "--csv", missing + ".csv", "--f0_path", missing + ".yaml", "--metrics", "mcd", metric])
    with pytest.raises(ValueError, match="spkemb_checkpoint"):
        cli.main(["--wavdir", missing, "--csv", missing + ".csv", "--f0_path", missing + ".yaml", "--metrics", "spkemb"])
    with pytest.raises(ValueError, match="unknown metric 'mos'"):
        cli.check_metrics(["mos"])
    assert cli.check_metrics(["mcd", "spkemb", "mcd"], "ckpt") == ["mcd", "spkemb"]


def test_calculate_gv_is_refused_by_name():
    from jatts_amd.evaluate import calculate_mcd_f0
    with pytest.raises(NotImplementedError, match="calculate_gv"):
        calculate_mcd_f0(np.zeros(8, np.float32), np.zeros(8, np.float32), 24000, 70, 400, calculate_gv=True)


def test_mean_line_has_the_reference_format():
    from jatts_amd.evaluate import format_mean
    means = {"MCD": 5.12345, "F0RMSE": 23.45678, "F0CORR": 0.87654, "DDUR": 0.12345}
    # evaluate.py:300-303, :311: f"MCD = {:.2f}", f"F0RMSE = {:.3f}", f"F0CORR = {:.3f}", f"DDUR = {:.3f}" joined by "; " behind "Mean "
    assert format_mean(means) == "Mean MCD = 5.12; F0RMSE = 23.457; F0CORR = 0.877; DDUR = 0.123"
    assert format_mean(means, 0.98765) == "Mean MCD = 5.12; F0RMSE = 23.457; F0CORR = 0.877; DDUR = 0.123; SPKEMB SIM = 0.988"
    assert format_mean(dict(means, F0RMSE=float("nan"))) == "Mean MCD = 5.12; F0RMSE = nan; F0CORR = 0.877; DDUR = 0.123"
    assert format_mean(None, 0.5) == "Mean SPKEMB SIM = 0.500"


def test_table_is_sorted_by_sample_id_and_aligned():
    from jatts_amd.bin.evaluate import format_table
    t = format_table(["b2", "a10", "a9"], [("MCD", ".2f", {"b2": 1.0, "a10": 22.333, "a9": 3.0})]).split("\n")
    assert [r.split()[0] for r in t[1:]] == ["a10", "a9", "b2"] and t[0].split() == ["Sample", "ID", "MCD"]
    assert len({len(r) for r in t}) == 1


def test_metrics_from_sums_matches_numpy_statistics():
    from jatts_amd.evaluate import metrics_from_sums
    rng = np.random.default_rng(3)
    x, y = 100.0 + 50.0 * rng.random(200), 100.0 + 50.0 * rng.random(200)
    terms = rng.random(150)
    f0 = [200.0, 0.0, x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(), ((x - y) ** 2).sum()]
    mcd, rmse, corr = metrics_from_sums([150.0, terms.sum()], f0)
    assert mcd == pytest.approx(10.0 / np.log(10.0) * terms.mean(), rel=1e-14)
    assert rmse == pytest.approx(np.sqrt(np.mean((x - y) ** 2)), rel=1e-14)
    assert corr == pytest.approx(np.corrcoef(x, y)[0, 1], abs=1e-10)
    assert all(np.isnan(v) for v in metrics_from_sums([150.0, terms.sum()], None)[1:])
    same = [200.0, 0.0, x.sum(), x.sum(), (x * x).sum(), (x * x).sum(), (x * x).sum(), 0.0]
    assert metrics_from_sums([1.0, 0.0], same) == (0.0, 0.0, 1.0)
    assert ER.metrics_from_sums([150.0, terms.sum()], f0) == (mcd, rmse, corr)


def test_pair_geometry_offsets_do_not_overlap():
    from jatts_amd import hip
    g = hip.PairGeometry([3, 0, 17], [5, 4, 1], gap=7)
    assert g.c_off == [7, 7 + 15 + 7, 7 + 15 + 7 + 0 + 7] and g.c_total == g.c_off[2] + 17 + 7
    assert g.d_off == [7, 7 + 3 + 7, 7 + 3 + 7 + 0 + 7] and g.d_total == g.d_off[2] + 17 + 7
    assert g.p_off == [7, 7 + 7 + 7, 7 + 7 + 7 + 3 + 7] and g.p_total == g.p_off[2] + 17 + 7
    assert g.a_row0 == [0, 3, 3] and g.b_row0 == [0, 5, 9] and (g.max_n, g.max_m) == (17, 5)
