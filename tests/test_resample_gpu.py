"""GPU: the sample-rate converter of jatts_amd.features (jatts_resample, jatts_wave_gain_peak) against tests/golden/resample_kat.npz.

What is pinned: scipy.signal.resample_poly in float64 on our float32 taps (tests/golden/make_golden_resample.py), and the taps on
scipy.signal.firwin (tests/test_resample_cpu.py).  What is NOT pinned: librosa.load(sr=...) / soxr_hq, absent from the build environment.

Three kinds of check:
  impulses  x = a * delta_p: one non-zero product plus exact zeros has no rounding, so the output IS a * taps, bit for bit;
  golden    for every output |y - y64| <= 1.01 * K * 2^-24 * S[m] + K * 2^-149, S = sum |h| |x|: the worst-case bound of any ordered f32
            sum of K products (each fma rounds once, relative 2^-24 of a partial sum that |.|-sums bound by S; K of them, 1.01 for the
            second-order terms; K * 2^-149 for products in the subnormal range) -- derived, not measured.  A misplaced tap errs by S itself;
  class     max_m |y - y64| / S <= 2 * E32, E32 the same measure of scipy's own float32 run (the fixture's): the same arithmetic in a
            different, shorter-chained order.  A CPU emulation of a two-level order (64-term chains, added in order) on the fixture gives
            0.58 - 1.17 x E32; measured on an MI355X: 0.57 - 1.17 x E32 and at most 0.049 of the bound (profiles/r17_notes.md).
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -77.25


def _kat():
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "resample_kat.npz"))
    return z, json.loads(str(z["cases"]))


CASE_NAMES = [c["name"] for c in _kat()[1]]
# 16 -> 48 kHz is Nbp 64: TWO table-column tiles, the (column tile, block tile) deal with both slots live, which no fixture case reaches
# (Nbp 32, 96, 160).  The design constants of the fixture's zeros = 64 cases; no golden arrays, so only the tests that need none take it.
EXTRA_CASES = [dict(next(c for c in _kat()[1] if c["zeros"] == 64), name="16k_48k", sr_in=16000, sr_out=48000, up=3, down=1)]
NO_GOLDEN_NAMES = CASE_NAMES + [c["name"] for c in EXTRA_CASES]
_CTX = {}


def _ctx(name, cuda):
    """Per case: (case dict, Resampler, host taps, geometry); shared by the tests, never modified."""
    if name not in _CTX:
        from jatts_amd import features as F
        c = next(c for c in _kat()[1] + EXTRA_CASES if c["name"] == name)
        rs = F.Resampler(cuda, c["sr_in"], c["sr_out"], zeros=c["zeros"], rolloff=c["rolloff"], beta=c["beta"])
        _CTX[name] = (c, rs, rs.taps.cpu().numpy(), rs.geometry)
    return _CTX[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(rs, waves, cuda, guard=0):
    """One jatts_resample launch into a sentinel-filled buffer with ``guard`` extra floats -> (outputs per utterance, guard region)."""
    from jatts_amd import features as F
    from jatts_amd import hip
    pw = F.PackedWaves.from_list([torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)) for w in waves], cuda)
    n_out = [rs.out_len(n) for n in pw.lens]
    cu_out = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    buf = torch.full((int(cu_out[-1]) + guard,), SENTINEL, dtype=torch.float32, device=cuda)
    hip.resample(pw.cu, hip.h2d([int(v) for v in cu_out], torch.int32, cuda), pw.lens, n_out, pw.x, rs.table, rs.up, rs.down, rs.half_len,
                 out=buf)
    y = buf.cpu().numpy()
    return [y[cu_out[b]:cu_out[b + 1]] for b in range(len(n_out))], y[cu_out[-1]:]


@pytest.mark.parametrize("name", NO_GOLDEN_NAMES)
def test_impulses_reproduce_the_taps_bit_for_bit(cuda, name):
    c, rs, taps, g = _ctx(name, cuda)
    up, down, half_len, hop_b, lead = rs.up, rs.down, rs.half_len, g["hop_b"], g["L"]
    n_in = 66 * hop_b + 3
    q1 = -(-lead // hop_b) + 1
    ps = sorted({0, 1, lead, n_in - 1,
                 q1 * hop_b - lead + 63, q1 * hop_b - lead + 64,            # both sides of a 64-sample chunk edge of block q1's operand
                 5 * hop_b - 1, 5 * hop_b,                                  # both sides of a block edge
                 64 * hop_b - 1, 64 * hop_b})                               # ... and of a workgroup's 64 blocks
    assert all(0 <= p < n_in for p in ps)
    waves, want = [], []
    n_out = rs.out_len(n_in)
    m = np.arange(n_out, dtype=np.int64)
    for amp in (1.0, 0.5):
        for p in ps:
            x = np.zeros(n_in, np.float32)
            x[p] = amp
            j = m * down - p * up + half_len
            ok = (j >= 0) & (j < taps.size)
            waves.append(x)
            want.append(np.where(ok, np.float32(amp) * taps[np.clip(j, 0, taps.size - 1)], np.float32(0.0)).astype(np.float32))
    got, guard = _launch(rs, waves, cuda, guard=4096)
    for i, (y, w) in enumerate(zip(got, want)):
        assert w.any() and np.array_equal(_bits(y), _bits(w)), (name, i, ps[i % len(ps)])
    assert (guard == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_golden_every_output_within_the_ordered_sum_bound_and_twice_scipys_float32(cuda, name):
    z, _ = _kat()
    c, rs, taps, g = _ctx(name, cuda)
    xs = [z["x_noise"], z["x_chirp"]]
    ys = rs([torch.from_numpy(x).to(cuda) for x in xs])
    k_rows = g["K"]
    worst = 0.0
    for key, y in zip(("noise", "chirp"), ys):
        y64, s = z[f"{name}_{key}_y64"], z[f"{name}_{key}_S"]
        assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == y64.shape
        err = np.abs(y.double().cpu().numpy() - y64)
        bound = 1.01 * k_rows * 2.0 ** -24 * s + k_rows * 2.0 ** -149
        print(f"{name} {key}: max |y - y64| / bound = {float((err / bound).max()):.4f}")
        assert (err <= bound).all(), (name, key, float((err / bound).max()))
        worst = max(worst, float((err / s).max()))
    e32 = float(z[f"{name}_E32"])
    print(f"{name}: max |y - y64| / S = {worst:.3e} = {worst / e32:.3f} x E32 ({e32:.3e})")
    assert worst <= 2.0 * e32, (name, worst, e32)


@pytest.mark.parametrize("name", NO_GOLDEN_NAMES)
def test_edges_and_ragged_batches_are_bit_identical_to_single_launches(cuda, name):
    from scipy.signal import resample_poly
    c, rs, taps, g = _ctx(name, cuda)
    hop_b, lead, k_rows = g["hop_b"], g["L"], g["K"]
    lens = [1, 2, hop_b - 1, hop_b, hop_b + 1, lead, lead + 1, k_rows - 1, k_rows, 64 * hop_b - 1, 64 * hop_b + 1]
    rng = np.random.default_rng(len(name))
    waves = [(0.1 * rng.standard_normal(lens[i % len(lens)])).astype(np.float32) for i in range(70)]
    got, guard = _launch(rs, waves, cuda, guard=8192)
    assert (guard == np.float32(SENTINEL)).all()                               # nothing written past the last n_out
    h64 = taps.astype(np.float64)
    for i, (x, y) in enumerate(zip(waves, got)):
        assert y.shape[0] == -(-x.shape[0] * rs.up // rs.down)
        if i < 2 * len(lens):                                                   # every length twice: against the definition
            x64 = x.astype(np.float64)
            y64 = resample_poly(x64, rs.up, rs.down, window=h64 / rs.up)
            s = resample_poly(np.abs(x64), rs.up, rs.down, window=np.abs(h64) / rs.up)
            assert (np.abs(y.astype(np.float64) - y64) <= 1.01 * k_rows * 2.0 ** -24 * s + k_rows * 2.0 ** -149).all(), (name, i, x.shape[0])
        solo, sguard = _launch(rs, [x], cuda, guard=1024)
        assert np.array_equal(_bits(solo[0]), _bits(y)), (name, i, x.shape[0])  # its place in the batch does not matter
        assert (sguard == np.float32(SENTINEL)).all()                           # nothing written past n_out


def test_equal_rates_are_the_identity(cuda):
    from jatts_amd import features as F
    x = torch.randn(1000, generator=torch.Generator().manual_seed(0)).to(cuda)
    rs = F.Resampler(cuda, 24000, 24000)
    out = rs([x])
    assert out[0] is x and F.resample(x, 22050, 22050) is x
    pw = F.PackedWaves(x, [400, 600])
    assert rs(pw) is pw


def test_one_shot_resample_equals_the_resampler(cuda):
    from jatts_amd import features as F
    z, _ = _kat()
    x = torch.from_numpy(z["x_noise"]).to(cuda)
    a = F.resample(x, 48000, 24000)
    b = F.Resampler(cuda, 48000, 24000)([x])[0]
    pw = F.resample(F.PackedWaves(torch.cat([x, x[:77]]), [x.numel(), 77]), 48000, 24000)
    assert torch.equal(a, b) and pw.lens == [1001, 39] and torch.equal(pw.split()[0], a)


def test_wave_gain_peak_is_one_multiply_and_exact_maxima(cuda):
    from jatts_amd import hip
    rng = np.random.default_rng(3)
    lens = [1, 63, 1024, 1025, 5000, 33333]
    waves = [rng.uniform(-0.9, 0.9, n).astype(np.float32) for n in lens]
    waves[4][4999] = -0.97                                                      # the peak in the last element, negative
    cu = [0] + [int(v) for v in np.cumsum(lens)]
    for gain in (1.0, 1.7, 0.3):
        y = torch.from_numpy(np.concatenate(waves)).to(cuda)
        peak = hip.wave_gain_peak(hip.h2d(cu, torch.int32, cuda), len(lens), y, gain).cpu().numpy()
        y = y.cpu().numpy()
        for b, w in enumerate(waves):
            want = w * np.float32(gain)
            assert np.array_equal(_bits(y[cu[b]:cu[b + 1]]), _bits(want)), (gain, b)
            assert peak[b, 0] == np.abs(w).max() and peak[b, 1] == np.abs(want).max(), (gain, b)


def test_cpu_tensors_raise(cuda):
    from jatts_amd import features as F
    from jatts_amd._abi import JattsHipError
    x = torch.zeros(100)
    with pytest.raises(JattsHipError):
        F.Resampler("cpu", 48000, 24000)
    with pytest.raises(JattsHipError):
        F.Resampler(cuda, 48000, 24000)([x])
    with pytest.raises(JattsHipError):
        F.resample(x, 48000, 24000)
    with pytest.raises(JattsHipError):
        F.PackedWaves(x, [100])
