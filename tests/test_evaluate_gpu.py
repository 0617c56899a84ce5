"""GPU: the stage-5 kernels of csrc/evaluate.hip against the float64 / exact restatements of tests/evaluate_reference.py,
then jatts_amd.evaluate end to end on synthetic voiced signals and the jatts_amd.bin.evaluate CLI on a toy set.

jatts_frame_select and jatts_dtw are held to EQUAL results (index lists; path arrays, length and final cost bit for bit), jatts_pairwise_dist,
jatts_dtw_path_stats and the cepstra to bounds worked out from the number formats, the whole chain to the float64 chain within four times
the difference measured on an MI355X (profiles/r29_notes.md)."""
import csv
import json
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
import yaml

import evaluate_reference as ER
import pitch_reference as PR
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
POISON = -0x5A5A5A5B
# |MCD - float64 chain| (dB) and |F0RMSE - float64 chain| (Hz) on the end-to-end pairs: four times the largest difference measured on an
# MI355X over the six pairs of test_end_to_end_against_the_float64_chain (profiles/r29_notes.md holds every observed value).  Observed:
# MCD 1.734e-06 dB (24 kHz, pair 0), F0RMSE 1.443e-06 Hz (22.05 kHz, pair 1); the paths equal the float64 chain's on all six.
MCD_TOL_DB = 4 * 1.734e-6
F0RMSE_TOL_HZ = 4 * 1.443e-6


def _i32(t):
    return t.cpu().numpy()


# ---- jatts_frame_select
LENS = (1, 63, 64, 65, 257, 1000)


def _select_case(kind):
    rng = np.random.default_rng({"mean": 1, "mean_none": 2, "mean_all": 3, "pos": 4, "pos_none": 5, "pos_all": 6, "max": 7, "max_none": 8,
                                 "max_all": 9}[kind])
    vals = []
    for n in LENS:
        if kind == "mean":
            v = np.exp(rng.normal(0.0, 2.0, n))
        elif kind in ("mean_none", "mean_all", "pos_all"):
            v = 1.0 + rng.random(n)
        elif kind == "pos":
            v = np.where(rng.random(n) < 0.4, 0.0, 50.0 + 300.0 * rng.random(n))
        elif kind in ("pos_none", "max_none"):
            v = np.zeros(n)
        else:
            v = 10.0 ** rng.uniform(-9.0, 0.0, n)
        vals.append(v.astype(np.float32))
    mode, factor = {"mean": (0, 0.5), "mean_none": (0, 10.0), "mean_all": (0, 0.1), "pos": (1, 0.0), "pos_none": (1, 0.0), "pos_all": (1, 0.0),
                    "max": (2, 1e-6), "max_none": (2, 1e-6), "max_all": (2, 1e-12)}[kind]
    return vals, mode, factor


@pytest.mark.parametrize("kind", ["mean", "mean_none", "mean_all", "pos", "pos_none", "pos_all", "max", "max_none", "max_all"])
def test_frame_select_equals_the_restatement(cuda, lib, kind):
    from jatts_amd import hip
    vals, mode, factor = _select_case(kind)
    # a condition on the INPUTS, asserted on the reference side first: in float64 no frame lies within a relative 1e-9 of the threshold
    for v in vals:
        v64 = v.astype(np.float64)
        thr = factor * v64.mean() if mode == 0 else 0.0 if mode == 1 else factor * v64.max()
        assert ER.threshold_margin(v, thr) > 1e-9
    rb = hip.RaggedBatch(LENS, cuda)
    x = torch.from_numpy(np.concatenate(vals)).to(cuda)
    runs = [hip.frame_select(rb, x, mode, factor) for _ in range(2)]
    if mode == 2:
        got = _i32(runs[0][0])
        assert np.array_equal(got, _i32(runs[1][0])) and runs[0][1] is None
        want = [ER.select_max(v, factor) for v in vals]
        assert got.tolist() == [list(w) for w in want]
        assert all(w == (-1, -1) for w in want) == (kind == "max_none") and (kind != "max_all" or all(w == (0, n - 1) for w, n in zip(want, LENS)))
        return
    count, idx = _i32(runs[0][0]), _i32(runs[0][1])
    count2, idx2 = _i32(runs[1][0]), _i32(runs[1][1])
    want = [ER.select_mean(v, factor) if mode == 0 else ER.select_positive(v) for v in vals]
    assert count.tolist() == [w.size for w in want] and np.array_equal(count, count2)
    for b, w in enumerate(want):
        o = rb.cu_host[b]
        assert np.array_equal(idx[o:o + w.size], w) and np.array_equal(idx2[o:o + w.size], w), (kind, b)
    if kind.endswith("_none"):
        assert count.sum() == 0
    if kind.endswith("_all"):
        assert count.tolist() == list(LENS)
    # the packed rows: jatts_gather_rows over a matrix of pitch 7 (4 columns used) and over a 1-D track
    rb_out = hip.RaggedBatch(count.tolist(), cuda)
    src = torch.arange(rb.total * 7, dtype=torch.float32, device=cuda).view(-1, 7)
    got = hip.gather_rows(rb, runs[0][1], rb_out, src, dim=4).cpu().numpy()
    got1 = hip.gather_rows(rb, runs[0][1], rb_out, src[:, 0].contiguous()).cpu().numpy()
    rows = np.concatenate([rb.cu_host[b] + w for b, w in enumerate(want)]).astype(np.int64) if rb_out.total else np.zeros(0, np.int64)
    assert got.shape == (rb_out.total, 4) and np.array_equal(got, src.cpu().numpy()[rows, :4]) and np.array_equal(got1, src.cpu().numpy()[rows, 0])


# ---- jatts_pairwise_dist
@pytest.mark.parametrize("dim", [1, 40, 64])
def test_pairwise_dist_against_float64(cuda, lib, dim):
    """One ragged launch over the four shapes; the rows sit in matrices of pitch dim + 3.  |c - c64| <= (dim + 3) 2^-24 c64: one rounding per
    difference, per square and per add, plus the root (halved by the root itself).  Identical rows give exactly 0."""
    from jatts_amd import hip
    shapes = ((1, 1), (1, 300), (257, 3), (130, 257))
    rng = np.random.default_rng(dim)
    a = rng.normal(0.0, 3.0, (sum(n for n, _ in shapes), dim + 3)).astype(np.float32)
    b = rng.normal(0.0, 3.0, (sum(m for _, m in shapes), dim + 3)).astype(np.float32)
    geo = hip.PairGeometry([n for n, _ in shapes], [m for _, m in shapes], gap=3)
    for p in range(len(shapes)):
        b[geo.b_row0[p] + shapes[p][1] - 1, :dim] = a[geo.a_row0[p], :dim]       # pair p: the first row of a equals the last row of b
    out = torch.full((geo.c_total,), float("nan"), dtype=torch.float32, device=cuda)
    c = hip.pairwise_dist(geo, torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), dim, out=out).cpu().numpy()
    seen = np.zeros(geo.c_total, dtype=bool)
    worst = 0.0
    for p, (n, m) in enumerate(shapes):
        got = c[geo.c_off[p]:geo.c_off[p] + n * m].reshape(n, m).astype(np.float64)
        seen[geo.c_off[p]:geo.c_off[p] + n * m] = True
        ref = ER.pairwise_dist(a[geo.a_row0[p]:geo.a_row0[p] + n, :dim], b[geo.b_row0[p]:geo.b_row0[p] + m, :dim])
        assert got[0, m - 1] == 0.0 and ref[0, m - 1] == 0.0
        err = np.abs(got - ref)
        worst = max(worst, float(np.max(err / np.maximum(ref, 1e-300) * (ref > 0))))
        assert (err <= (dim + 3) * U * ref).all(), (dim, n, m, float(err.max()))
    print(f"pairwise_dist dim {dim}: worst relative error {worst / U:.2f} x 2^-24 (bound {dim + 3})")
    assert np.isnan(c[~seen]).all()                                              # the gaps between the pairs keep their bits


# ---- jatts_dtw
def _dtw_buffers(geo, cuda, extra=2):
    mk = lambda n, dt: torch.full((n,), POISON, dtype=dt, device=cuda)      # noqa: E731
    return (mk(geo.d_total, torch.int32), mk(geo.p_total, torch.int32), mk(geo.p_total, torch.int32), mk(geo.n_pairs + extra, torch.int32),
            torch.full((geo.n_pairs + extra,), -7.25, dtype=torch.float64, device=cuda))


def _run_dtw(costs, cuda, gap=5):
    """One launch over ``costs`` (f32 matrices) with poisoned outputs -> per pair (path_i, path_j, total); asserts the poison outside the
    pairs' own output survives: the gaps, the unused tail of each path (capacity n + m - 1) and the entries behind the last pair."""
    from jatts_amd import hip
    geo = hip.PairGeometry([c.shape[0] for c in costs], [c.shape[1] for c in costs], gap=gap)
    flat = np.full(geo.c_total, np.nan, dtype=np.float32)
    for p, c in enumerate(costs):
        flat[geo.c_off[p]:geo.c_off[p] + c.size] = c.reshape(-1)
    bufs = _dtw_buffers(geo, cuda)
    plen, pi, pj, total = hip.dtw(geo, torch.from_numpy(flat).to(cuda), bufs)
    plen, pi, pj, total, dec = _i32(plen), _i32(pi), _i32(pj), total.cpu().numpy(), _i32(bufs[0])
    assert (plen[geo.n_pairs:] == POISON).all() and (total[geo.n_pairs:] == -7.25).all()
    keep_p, keep_d = np.ones(geo.p_total, dtype=bool), np.ones(geo.d_total, dtype=bool)
    out = []
    for p, c in enumerate(costs):
        L, o = int(plen[p]), geo.p_off[p]
        assert max(c.shape) <= L <= sum(c.shape) - 1
        keep_p[o:o + L] = False
        keep_d[geo.d_off[p]:geo.d_off[p] + c.shape[0] * ((c.shape[1] + 15) // 16)] = False
        out.append((pi[o:o + L], pj[o:o + L], float(total[p])))
    assert (pi[keep_p] == POISON).all() and (pj[keep_p] == POISON).all() and (dec[keep_d] == POISON).all()
    return out


def _dtw_costs(n, m, kind, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, m)) + 0.01).astype(np.float32) if kind == "random" else rng.integers(0, 3, (n, m)).astype(np.float32)


def _assert_same_path(got, c):
    pi, pj, total = ER.dtw_fast(c)
    assert got[2] == total, (c.shape, got[2], total)                             # the same float64 adds of the same f32 values: the same bits
    assert np.array_equal(got[0], pi) and np.array_equal(got[1], pj), c.shape


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (17, 1), (2, 300), (256, 256), (257, 255), (1000, 700)])
def test_dtw_is_bit_identical_to_the_restatement(cuda, lib, shape, kind):
    c = _dtw_costs(*shape, kind, shape[0] + 3 * shape[1])
    _assert_same_path(_run_dtw([c], cuda)[0], c)


def test_dtw_at_both_sides_of_every_row_slot_boundary(cuda, lib):
    """Thread t owns rows t + 256 m, m < 16: N = 256 m and 256 m + 1 for every m up to the cap of 4096 rows (each launch picks the smallest
    of the 1 / 2 / 4 / 8 / 16-slot instantiations that holds N), narrow matrices (M = 7 / 21: one and two decision words a row), tie-heavy
    and random costs alternating."""
    from jatts_amd import hip
    assert hip.dtw_max_rows() == 4096
    sizes = sorted({256 * m + d for m in range(1, 17) for d in (0, 1) if 256 * m + d <= 4096})
    assert len(sizes) == 31 and sizes[-1] == 4096
    for k, n in enumerate(sizes):
        c = _dtw_costs(n, 21 if k % 3 == 0 else 7, "ties" if k % 2 else "random", n)
        _assert_same_path(_run_dtw([c], cuda)[0], c)


def test_dtw_ragged_batch_of_five_pairs_in_one_launch(cuda, lib):
    shapes = ((300, 41), (1, 1), (513, 130), (40, 333), (77, 77))
    costs = [_dtw_costs(n, m, "ties" if p % 2 else "random", 11 + p) for p, (n, m) in enumerate(shapes)]
    got = _run_dtw(costs, cuda)
    for g, c in zip(got, costs):
        _assert_same_path(g, c)
    again = _run_dtw(costs, cuda)
    assert all(a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, again))
    # an empty side: L = 0 and nothing else written (the caller refuses such pairs; the kernel must not touch memory for them)
    from jatts_amd import hip
    geo = hip.PairGeometry([0, 5], [4, 0], gap=2)
    bufs = _dtw_buffers(geo, cuda)
    plen = _i32(hip.dtw(geo, torch.zeros(max(geo.c_total, 1), dtype=torch.float32, device=cuda), bufs)[0])
    assert plen[:2].tolist() == [0, 0] and (_i32(bufs[1]) == POISON).all() and (bufs[4].cpu().numpy() == -7.25).all()


def test_dtw_refuses_a_pair_over_the_row_cap_before_any_launch(cuda, lib):
    from jatts_amd import hip
    geo = hip.PairGeometry([4097], [2])
    bufs = _dtw_buffers(geo, cuda)
    with pytest.raises(ValueError, match="4096"):
        hip.dtw(geo, torch.zeros(geo.c_total, dtype=torch.float32, device=cuda), bufs)
    torch.cuda.synchronize()
    assert all((_i32(b) == POISON).all() for b in bufs[:4])                       # nothing ran
    with pytest.raises(hip._abi.JattsHipError):
        hip.dtw(hip.PairGeometry([3], [3]), torch.zeros(9, dtype=torch.float32))   # CPU tensors: refused as everywhere else


# ---- jatts_dtw_path_stats
def test_path_stats_against_float64_and_twice(cuda, lib):
    """Paths of the restated DTW on random costs; matrices of pitch 48 (40 columns used) and tracks.  The kernel's terms are the float64
    terms of ER.path_terms bit for bit (same operations, same order), so only the order of the sum differs: every sum within
    L 2^-52 sum |terms| of numpy's float64 sum."""
    from jatts_amd import hip
    shapes = ((1, 1), (300, 257), (40, 700), (1000, 900))
    rng = np.random.default_rng(5)
    geo = hip.PairGeometry([n for n, _ in shapes], [m for _, m in shapes], gap=4)
    a = rng.normal(0.0, 2.0, (sum(geo.n), 48)).astype(np.float32)
    b = rng.normal(0.0, 2.0, (sum(geo.m), 48)).astype(np.float32)
    x, y = (80.0 + 200.0 * rng.random(sum(geo.n))).astype(np.float32), (80.0 + 200.0 * rng.random(sum(geo.m))).astype(np.float32)
    pi_all, pj_all = np.full(geo.p_total, POISON, dtype=np.int32), np.full(geo.p_total, POISON, dtype=np.int32)
    plen, paths = [], []
    for p, (n, m) in enumerate(shapes):
        pi, pj, _ = ER.dtw_fast(_dtw_costs(n, m, "random", 70 + p))
        pi_all[geo.p_off[p]:geo.p_off[p] + pi.size], pj_all[geo.p_off[p]:geo.p_off[p] + pi.size] = pi, pj
        plen.append(pi.size)
        paths.append((pi, pj))
    dev = [torch.from_numpy(v).to(cuda) for v in (np.array(plen, dtype=np.int32), pi_all, pj_all, a, b, x, y)]
    runs = [hip.dtw_path_stats(geo, dev[0], dev[1], dev[2], a=dev[3], b=dev[4], dim=40, x=dev[5], y=dev[6]).cpu().numpy() for _ in range(2)]
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))
    only_m = hip.dtw_path_stats(geo, dev[0], dev[1], dev[2], a=dev[3], b=dev[4], dim=40).cpu().numpy()
    only_t = hip.dtw_path_stats(geo, dev[0], dev[1], dev[2], x=dev[5], y=dev[6]).cpu().numpy()
    assert np.array_equal(only_m[:, 1], runs[0][:, 1]) and (only_m[:, 2:] == 0).all()
    assert np.array_equal(only_t[:, 2:], runs[0][:, 2:]) and (only_t[:, 1] == 0).all()
    for p, (pi, pj) in enumerate(paths):
        t = ER.path_terms(pi, pj, a[geo.a_row0[p]:, :40], b[geo.b_row0[p]:, :40], x[geo.a_row0[p]:], y[geo.b_row0[p]:])
        L = pi.size
        assert runs[0][p, 0] == L
        for q, name in enumerate(ER.STAT_ORDER):
            want, mag = float(t[name].sum()), float(np.abs(t[name]).sum())
            assert abs(runs[0][p, 1 + q] - want) <= L * 2.0 ** -52 * mag, (p, name, runs[0][p, 1 + q], want)


# ---- the synthetic voiced signals of the end-to-end tests
def voiced_signal(fs, seconds=1.2, f_start=120.0, f_end=160.0, lead=0.0, seed=0):
    """A harmonic series on a linear F0 glide under a moving spectral envelope (two formant-like resonances that drift), ``lead`` seconds of
    exact zeros in front.  The series fills the band: every harmonic below 0.49 fs sounds (floor 0.02 of the envelope's peak), so that no
    mel bin is empty.  In an EMPTY band the log-mel holds the arithmetic's own floor -- f32 rounding at 1e-7 of the frame's peak on the GPU,
    the window's side lobes at 1e-9 in float64 -- and the logarithm turns that into nepers: a first version of these signals stopped at
    0.45 fs x the glide's lowest / highest F0 and measured |MCD - float64 chain| = 0.134 dB (24 kHz) and 0.137 dB (22.05 kHz) from the top
    mel bins alone, with identical paths (profiles/r29_notes.md).  Speech has a noise floor in every band."""
    n = int(round(seconds * fs))
    t = np.arange(n) / fs
    f0 = f_start + (f_end - f_start) * t / seconds
    phase = 2.0 * np.pi * np.cumsum(f0) / fs
    rng = np.random.default_rng(seed)
    f1, f2 = 500.0 + 300.0 * np.sin(2.0 * np.pi * 1.5 * t), 1800.0 + 600.0 * np.cos(2.0 * np.pi * 1.1 * t)
    x = np.zeros(n)
    for h in range(1, int(0.49 * fs / min(f_start, f_end)) + 1):
        fh = h * f0
        env = np.exp(-0.5 * ((fh - f1) / 250.0) ** 2) + 0.5 * np.exp(-0.5 * ((fh - f2) / 400.0) ** 2) + 0.02
        x += np.where(fh < 0.49 * fs, env, 0.0) * np.sin(h * phase + rng.uniform(0.0, 2.0 * np.pi))
    x *= (0.55 + 0.45 * np.sin(2.0 * np.pi * 2.3 * t + 0.3)) * 0.5 / np.abs(x).max()
    return np.concatenate([np.zeros(int(round(lead * fs))), x]).astype(np.float32)


F0MIN, F0MAX = 70.0, 400.0
_PAIRS = {}


def pairs_of(fs):
    """Three (x, y) pairs at ``fs``: y = another glide rate behind 0.25 s of zeros; built once per rate"""
    if fs not in _PAIRS:
        _PAIRS[fs] = [(voiced_signal(fs, f_start=110.0 + 15.0 * k, f_end=150.0 + 20.0 * k, seed=k),
                       voiced_signal(fs, f_start=110.0 + 15.0 * k, f_end=170.0 + 25.0 * k, lead=0.25, seed=k)) for k in range(3)]
    return _PAIRS[fs]


def float64_features(x, fs):
    """The front end in float64 (numpy FFT over the package's own frame geometry, window and mel matrix: host constants pinned in
    tests/test_features_gpu.py) -> (cepstra (T, 40), power sum (T,), f0 (T,) from tests/pitch_reference.py)"""
    from jatts_amd.features import stft as S
    hop = int(round(fs * 0.005))
    x64 = x.astype(np.float64)
    spec = np.fft.rfft(x64[S.frame_indices(x.size, 1024, hop)] * S.padded_window("hann", None, 1024)[None, :], axis=1)
    mag = np.abs(spec)
    logmel = np.log(np.maximum(1e-10, mag @ S.mel_filterbank(fs, 1024, 80, 70.0, fs / 2.0)))
    return ER.cepstra(logmel), (mag ** 2).sum(axis=1), PR.analyse(x64, fs, 2048, hop, F0MIN, F0MAX)["f0"]


@pytest.mark.parametrize("fs", [24000, 22050])
def test_cepstra_equal_the_float64_dct_of_the_own_logmel(cuda, lib, fs):
    """|c - sum_k w_ck m_k| <= 81 2^-24 sum_k |w_ck| |m_k| per coefficient: the weight's rounding and the 80 accumulations of the exact-f32
    chain, m the extractor's own f32 log-mel (pinned in tests/test_features_gpu.py)."""
    from jatts_amd.evaluate import Evaluator
    ev = Evaluator(cuda)
    x, y = pairs_of(fs)[0]
    rb, cep, pow_sum, logmel = ev.cepstra([x, y], fs)
    hop = int(round(fs * 0.005))
    assert rb.lens == [1 + x.size // hop, 1 + y.size // hop] and cep.shape == (rb.total, 40) and pow_sum.shape == (rb.total,)
    m = logmel[:, :80].cpu().numpy().astype(np.float64)
    w = ER.dct_matrix(80, 40)
    err = np.abs(cep.cpu().numpy().astype(np.float64) - m @ w.T)
    bound = 81 * U * (np.abs(m) @ np.abs(w).T)
    print(f"cepstra fs {fs}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    from jatts_amd._abi import JattsHipError
    with pytest.raises(JattsHipError):
        ev.active_frames(rb, pow_sum.cpu())                                      # CPU tensors: refused as everywhere else


@pytest.mark.parametrize("fs", [24000, 22050])
def test_identical_waves_give_zero_distance(cuda, lib, fs):
    from jatts_amd.evaluate import calculate_mcd_f0
    x = pairs_of(fs)[0][0]
    r = calculate_mcd_f0(x, x, fs, F0MIN, F0MAX)
    assert r["MCD"] == 0.0 and r["F0RMSE"] == 0.0 and abs(r["F0CORR"] - 1.0) <= 1e-12 and r["DDUR"] == 0.0


@pytest.mark.parametrize("fs", [24000, 22050])
def test_batch_equals_single_calls_and_paths_are_monotone(cuda, lib, fs):
    from jatts_amd.evaluate import Evaluator
    ev = Evaluator(cuda)
    pairs = pairs_of(fs)
    batch = ev.evaluate_batch(pairs, fs, F0MIN, F0MAX, want_paths=True)
    for (x, y), r in zip(pairs, batch):
        single = ev.evaluate_batch([(x, y)], fs, F0MIN, F0MAX)[0]
        for k in ("MCD", "F0RMSE", "F0CORR", "DDUR"):
            assert np.float64(single[k]).view(np.uint64) == np.float64(r[k]).view(np.uint64), k      # bit for bit
            assert np.isfinite(r[k])
        assert r["DDUR"] <= 2 * 512 / fs
        pi, pj = r["path"]
        assert pi[0] == 0 and pj[0] == 0 and pi.size == pj.size
        di, dj = np.diff(pi), np.diff(pj)
        assert ((di >= 0) & (dj >= 0) & (di <= 1) & (dj <= 1) & (di + dj >= 1)).all()
        rb, _, pow_sum, _ = ev.cepstra([x, y], fs)
        n_act = ev.active_frames(rb, pow_sum)[0].cpu().tolist()
        assert (int(pi[-1]), int(pj[-1])) == (n_act[0] - 1, n_act[1] - 1) and 0 < n_act[1] < rb.lens[1]      # ends at (N - 1, M - 1); y's lead is cut


def test_silent_wave_is_refused_by_sample_name(cuda, lib):
    from jatts_amd.evaluate import Evaluator
    x = pairs_of(24000)[0][0]
    with pytest.raises(ValueError, match="utt_silent"):
        Evaluator(cuda).evaluate_batch([(x, x, "utt_ok"), (x, np.zeros(20000, np.float32), "utt_silent")], 24000, F0MIN, F0MAX)


@pytest.mark.parametrize("fs", [24000, 22050])
def test_end_to_end_against_the_float64_chain(cuda, lib, fs):
    """MCD and F0RMSE against the float64 restatement of the WHOLE chain (float64 STFT, log-mel, DCT, pitch, selection, DTW, sums).  The
    difference comes from f32 features moving near-tie path decisions and cannot be derived: the bounds are four times the largest
    difference measured on an MI355X (profiles/r29_notes.md)."""
    from jatts_amd.evaluate import Evaluator
    got = Evaluator(cuda).evaluate_batch(pairs_of(fs), fs, F0MIN, F0MAX)
    worst = []
    for k, ((x, y), r) in enumerate(zip(pairs_of(fs), got)):
        cx, px, fx = float64_features(x, fs)
        cy, py, fy = float64_features(y, fs)
        mcd, rmse, corr, _ = ER.evaluate_chain(cx, cy, px, py, fx, fy)
        print(f"end to end fs {fs} pair {k}: MCD {r['MCD']:.6f} (float64 chain {mcd:.6f}, |d| {abs(r['MCD'] - mcd):.3e} dB), "
              f"F0RMSE {r['F0RMSE']:.6f} ({rmse:.6f}, |d| {abs(r['F0RMSE'] - rmse):.3e} Hz), F0CORR {r['F0CORR']:.6f} ({corr:.6f})")
        worst.append((abs(r["MCD"] - mcd), abs(r["F0RMSE"] - rmse)))
    assert max(w[0] for w in worst) <= MCD_TOL_DB and max(w[1] for w in worst) <= F0RMSE_TOL_HZ, worst


# ---- the CLI
def _write_wav(path, x, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())


def test_evaluate_cli_on_a_toy_set(cuda, lib, tmp_path):
    """Four pairs (generated at 24 kHz, ground truth at 48 kHz, so the ground truth passes through the resampler; one row cut by start / end),
    two speakers with their own f0 ranges: the Mean line parses, --json equals evaluate_batch, the table is sorted by id."""
    from jatts_amd.evaluate import Evaluator
    from jatts_amd.features import read_audio_batch
    from jatts_amd.wavio import decode_wav
    wavdir = tmp_path / "wav"
    wavdir.mkdir()
    f0 = {"spkA": {"f0min": 70, "f0max": 300}, "spkB": {"f0min": 80, "f0max": 400}}
    rows = []
    for k, sid in enumerate(("utt_c", "utt_a", "utt_d", "utt_b")):
        _write_wav(wavdir / f"{sid}.wav", voiced_signal(24000, 0.5 + 0.05 * k, 120.0 + 10.0 * k, 150.0 + 12.0 * k, seed=k), 24000)
        _write_wav(tmp_path / f"gt_{sid}.wav", voiced_signal(48000, 0.55 + 0.05 * k, 120.0 + 10.0 * k, 165.0 + 9.0 * k, lead=0.1, seed=k), 48000)
        rows.append({"sample_id": sid, "spk": "spkA" if k % 2 else "spkB", "wav_path": str(tmp_path / f"gt_{sid}.wav"),
                     "start": "0.05" if sid == "utt_a" else "", "end": "0.6" if sid == "utt_a" else ""})
    with open(tmp_path / "test.csv", "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0]))
        wr.writeheader()
        wr.writerows(rows)
    (tmp_path / "f0.yaml").write_text(yaml.safe_dump(f0))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-m", "jatts_amd.bin.evaluate", "--wavdir", str(wavdir), "--csv", str(tmp_path / "test.csv"), "--f0_path",
                        str(tmp_path / "f0.yaml"), "--metrics", "mcd", "--n_jobs", "4", "--batch-size", "3", "--json", str(tmp_path / "out.json")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stderr.splitlines()
    mean = [k for k, v in enumerate(lines) if "INFO: Mean " in v]
    defs = [k for k, v in enumerate(lines) if "own definition" in v and "INFO: " in v]
    assert len(mean) == 1 and len(defs) == 1 and defs[0] < mean[0] and any("--n_jobs 4 is accepted and unused" in v for v in lines)
    m = re.search(r"INFO: Mean MCD = (\d+\.\d\d); F0RMSE = (\d+\.\d{3}); F0CORR = (-?\d\.\d{3}); DDUR = (\d+\.\d{3})$", lines[mean[0]])
    assert m, lines[mean[0]]
    table = r.stdout.strip().splitlines()
    assert table[0].split() == ["Sample", "ID", "MCD", "F0RMSE", "F0CORR", "DDUR"]
    assert [t.split()[0] for t in table[1:]] == ["utt_a", "utt_b", "utt_c", "utt_d"]
    with open(tmp_path / "out.json") as f:
        out = json.load(f)
    ev = Evaluator(cuda)
    for row in rows:
        a, fs = decode_wav(str(wavdir / f"{row['sample_id']}.wav"))
        gt = read_audio_batch([(row["wav_path"], float(row["start"]) if row["start"] else None, float(row["end"]) if row["end"] else None)], fs)[0]
        want = ev.evaluate_batch([(a[:, 0], gt)], fs, float(f0[row["spk"]]["f0min"]), float(f0[row["spk"]]["f0max"]))[0]
        assert out["utterances"][row["sample_id"]] == want, row["sample_id"]
    for k, v in zip(("MCD", "F0RMSE", "F0CORR", "DDUR"), m.groups()):
        mean_k = float(np.mean([out["utterances"][s][k] for s in ("utt_c", "utt_a", "utt_d", "utt_b")]))
        assert out["mean"][k] == mean_k and v == format(mean_k, ".2f" if k == "MCD" else ".3f")
