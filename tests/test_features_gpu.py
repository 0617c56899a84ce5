"""GPU: jatts_amd.features (log-mel and energy on HIP) against tests/golden/logmel_kat.npz.

What is pinned: torch.stft in float64 (center=True, pad_mode="reflect", periodic Hann) and the transformers Slaney filterbank
(tests/golden/make_golden_logmel.py).  What is NOT pinned: librosa itself, which is absent from the build environment, so parity with
the reference's own extraction stays unverified.

Error measures, the same for the kernel and for the float32-FFT yardstick E32 the fixture stores (the reference's arithmetic class):
  lin = max over non-silent frames of max_m |mel - mel64| / max_m mel64[t]
  log = max |log_b mel - log_b mel64| over bins with mel64 >= 1e-3 x their frame's maximum
  en  = max relative energy error over non-silent frames
The kernel may be 8 x E32 on each, per setting (a 2048-term f32 sum against an FFT's log K depth), and never above the caps
lin 5e-6, log 1e-4, en 1e-5."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SETTINGS = {
    "a": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=2048, fmin=80, fmax=7600),
    "b": dict(sampling_rate=24000, fft_size=2048, hop_size=300, win_length=1200, fmin=80, fmax=7600),
    "c": dict(sampling_rate=22050, fft_size=1024, hop_size=256, win_length=None, fmin=None, fmax=None),
}
CAPS = np.array([5e-6, 1e-4, 1e-5])
EPS = 1e-10


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "logmel_kat.npz"))


def _waves(kat, name):
    lens = [int(v) for v in kat[f"{name}_lens"]]
    cu = np.concatenate([[0], np.cumsum(lens)])
    return [kat[f"{name}_wave"][cu[i]:cu[i + 1]] for i in range(len(lens))]


_RUNS = {}


def _run(kat, cuda, name, log_base=10.0):
    """One batched extraction per (setting, base), shared by the tests (never modified)."""
    key = (name, log_base)
    if key not in _RUNS:
        from jatts_amd.features import LogMelExtractor
        ex = LogMelExtractor(cuda, num_mels=80, log_base=log_base, **SETTINGS[name])
        waves = _waves(kat, name)
        rb, feats = ex(waves)
        en = ex.energy(waves)
        _RUNS[key] = (ex, waves, rb, feats, en, ex.mel(waves)[1])
    return _RUNS[key]


def _measures(mel, en, mel64, en64, silent, log=np.log10):
    live = ~silent
    top = mel64[live].max(axis=1, keepdims=True)
    lin = float((np.abs(mel[live] - mel64[live]) / top).max())
    strong = mel64[live] >= 1e-3 * top
    lg = float(np.abs(log(np.maximum(EPS, mel[live])) - log(np.maximum(EPS, mel64[live])))[strong].max())
    e = float((np.abs(en[live] - en64[live]) / en64[live]).max())
    return np.array([lin, lg, e])


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_logmel_and_energy_within_8x_the_float32_fft(kat, cuda, name):
    ex, waves, rb, feats, en, mel = _run(kat, cuda, name)
    assert rb.lens == [int(v) for v in kat[f"{name}_frames"]] == [1 + len(w) // ex.hop for w in waves]
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (rb.total, 128)
    assert not feats[:, 80:].any()                                            # padding columns exactly zero
    f = feats[:, :80].double().cpu().numpy()
    e = torch.cat(en).double().cpu().numpy()
    assert [int(v.numel()) for v in en] == rb.lens
    silent = kat[f"{name}_silent"]
    assert mel.dtype == torch.float32 and tuple(mel.shape) == (rb.total, 80)
    m = _measures(mel.double().cpu().numpy(), e, kat[f"{name}_mel64"], kat[f"{name}_energy64"], silent)
    # the log measure on the kernel's own logarithms
    live = ~silent
    mel64 = kat[f"{name}_mel64"]
    strong = mel64[live] >= 1e-3 * mel64[live].max(axis=1, keepdims=True)
    m[1] = float(np.abs(f[live] - kat[f"{name}_logmel64"][live])[strong].max())
    e32 = kat[f"{name}_e32"]
    print(f"features[{name}]: lin {m[0]:.3e} log {m[1]:.3e} en {m[2]:.3e} | E32 {e32[0]:.3e} {e32[1]:.3e} {e32[2]:.3e} | ratio "
          f"{m[0] / e32[0]:.2f} {m[1] / e32[1]:.2f} {m[2] / e32[2]:.2f}")
    assert (m <= 8.0 * e32).all() and (m <= CAPS).all(), (m, e32)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_silent_frames(kat, cuda, name):
    _, _, _, feats, en, _ = _run(kat, cuda, name)
    silent = torch.from_numpy(kat[f"{name}_silent"]).to(feats.device)
    assert int(silent.sum()) >= 2
    want = float(np.log10(np.float64(np.float32(EPS))))
    assert float((feats[silent][:, :80].double() - want).abs().max()) <= 1e-6
    floor = np.sqrt(np.float32(1e-10))
    got = torch.cat(en)[silent].cpu().numpy()
    assert (np.abs(got - floor) <= np.spacing(floor)).all()


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_batch_independent_and_repeatable(kat, cuda, name):
    ex, waves, rb, feats, en, mel = _run(kat, cuda, name)
    rb2, feats2 = ex(waves)
    en2 = ex.energy(waves)
    assert torch.equal(feats, feats2) and all(torch.equal(a, b) for a, b in zip(en, en2))
    for i, w in enumerate(waves):
        r1, f1 = ex([w])
        assert r1.lens == [rb.lens[i]]
        assert torch.equal(f1, feats[rb.cu_host[i]:rb.cu_host[i + 1]]), i
        assert torch.equal(ex.energy([w])[0], en[i]), i


@pytest.mark.parametrize("log_base", [None, 2.0])
def test_log_bases(kat, cuda, log_base):
    name = "c"
    _, _, rb, feats, _, _ = _run(kat, cuda, name, log_base)
    log = np.log if log_base is None else np.log2
    ref = log(np.maximum(EPS, kat[f"{name}_mel64"]))
    ref10 = _run(kat, cuda, name, 10.0)[3]
    f = feats[:, :80].double().cpu().numpy()
    silent = kat[f"{name}_silent"]
    live = ~silent
    mel64 = kat[f"{name}_mel64"]
    strong = mel64[live] >= 1e-3 * mel64[live].max(axis=1, keepdims=True)
    err = float(np.abs(f[live] - ref[live])[strong].max())
    scale = float(log(10.0))                                                   # log_b x = log_b 10 * log10 x
    bound = min(8.0 * float(kat[f"{name}_e32"][1]), CAPS[1]) * scale
    print(f"features[{name}, base {log_base}]: log {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert float(np.abs(f[silent] - log(np.float64(np.float32(EPS)))).max()) <= 1e-6 * scale
    # the same mel under another logarithm: agrees with the base-10 run, converted
    assert float((feats[:, :80].double() - ref10[:, :80].double() * scale).abs().max()) <= 2e-6 * scale
    assert not feats[:, 80:].any()


def test_logmelfilterbank_reference_signature(kat, cuda):
    from jatts_amd.features import logmelfilterbank
    name = "a"
    s = SETTINGS[name]
    _, waves, rb, feats, _, _ = _run(kat, cuda, name)
    i = 2
    y = logmelfilterbank(waves[i], s["sampling_rate"], fft_size=s["fft_size"], hop_size=s["hop_size"], win_length=s["win_length"],
                         window="hann", num_mels=80, fmin=s["fmin"], fmax=s["fmax"])
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (rb.lens[i], 80)
    assert np.array_equal(y, feats[rb.cu_host[i]:rb.cu_host[i + 1], :80].cpu().numpy())


def _token_average64(e, d):
    cum = np.concatenate([[0], np.cumsum(d)])
    out = []
    for a, z in zip(cum[:-1], cum[1:]):
        v = e[a:z][e[a:z] > 0.0]
        out.append(v.mean() if len(v) else 0.0)
    return np.array(out, dtype=np.float64)


def test_energy_forward_three_forms(kat, cuda):
    from jatts_amd.features import Energy
    name = "c"
    s = SETTINGS[name]
    waves = _waves(kat, name)
    i = 3                                                                       # the utterance with silent frames
    fr = [int(v) for v in kat[f"{name}_frames"]]
    cu = np.concatenate([[0], np.cumsum(fr)])
    e64 = kat[f"{name}_energy64"][cu[i]:cu[i + 1]]
    T = fr[i]
    plain = Energy(fs=s["sampling_rate"], n_fft=s["fft_size"], hop_length=s["hop_size"], use_token_averaged_energy=False, device=cuda)
    e = plain.forward(waves[i])
    assert isinstance(e, np.ndarray) and e.dtype == np.float32 and e.shape == (T,)
    tol = min(8.0 * float(kat[f"{name}_e32"][2]), CAPS[2])
    assert float((np.abs(e - e64) / e64).max()) <= tol
    short, long = plain.forward(waves[i], feat_length=T - 5), plain.forward(waves[i], feat_length=T + 4)
    assert np.array_equal(short, e[:T - 5]) and np.array_equal(long[:T], e) and long.shape == (T + 4,) and not long[T:].any()
    # token average over the padded form: a zero-duration token, and a last token that reaches into the zero padding
    tok = Energy(fs=s["sampling_rate"], n_fft=s["fft_size"], hop_length=s["hop_size"], use_token_averaged_energy=True,
                 reduction_factor=1, device=cuda)
    d = np.array([3, 0, 5, 1, T - 11, 2 + 4, 0], dtype=np.int64)                # sums to T + 4
    got = tok.forward(waves[i], feat_length=T + 4, durations=d)
    ref = _token_average64(np.concatenate([e64, np.zeros(4)]), d)
    assert got.dtype == np.float32 and got.shape == d.shape
    assert got[1] == 0.0 and got[6] == 0.0
    mean_tol = lambda n: (n + 1) * 2.0 ** -24                                   # n - 1 f32 adds of positives, a divide, and slack of one
    assert float((np.abs(got - ref) / np.maximum(ref, 1e-30))[ref > 0].max()) <= tol + mean_tol(int(d.max()))
    # a span of padded zeros only
    d2 = np.array([T, 4], dtype=np.int64)
    got2 = tok.forward(waves[i], feat_length=T + 4, durations=d2)
    assert got2[1] == 0.0 and abs(got2[0] - ref_mean(e64)) <= (tol + mean_tol(T)) * ref_mean(e64)
    with pytest.raises(ValueError):
        tok.forward(waves[i], feat_length=T + 4, durations=d[:-2])
    with pytest.raises(ValueError):
        tok.forward(waves[i], durations=d)                                     # sums to T + 4, the utterance has T frames


def ref_mean(e64):
    return float(e64[e64 > 0.0].mean())


def test_kernel_refusals_carry_the_entry_points_text(cuda):
    from jatts_amd import _abi, hip
    L = 3000
    x = torch.zeros(L, device=cuda)
    cu = torch.tensor([0, L], dtype=torch.int32, device=cuda)
    small = torch.zeros(64, device=cuda)                                        # never read: every call below is refused before a launch

    def call(n_fft, hop, ldo, n=L, frames=None, table=None):
        frames = 1 + n // max(hop, 1) if frames is None else frames
        t = table if table is not None else small
        return hip.stft_mag(hip.RaggedBatch([frames], cuda), cu, [n], x, t, n_fft, hop, ldo)

    with pytest.raises(_abi.JattsHipError, match="stft_mag: n_fft must be a multiple of 64, at most 2048"):
        call(4096, 300, 4160)
    tab = torch.zeros(1024, 2 * 544, device=cuda)
    with pytest.raises(_abi.JattsHipError, match="stft_mag: hop must lie in"):
        call(1024, 0, 576, table=tab)
    with pytest.raises(_abi.JattsHipError, match="stft_mag: hop must lie in"):
        call(1024, 1025, 576, table=tab)
    with pytest.raises(_abi.JattsHipError, match="stft_mag: ldo < n_bins"):
        call(1024, 256, 512, table=tab)
    with pytest.raises(_abi.JattsHipError, match="cannot be reflect-padded"):
        call(1024, 256, 576, n=512, table=tab)
    with pytest.raises(_abi.JattsHipError, match="frame geometry"):
        call(1024, 256, 576, frames=40, table=tab)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_fft,hop,win", [(64, 7, None), (128, 33, 100), (256, 64, None), (320, 77, 200)])
def test_other_tile_paths_against_float64(cuda, n_fft, hop, win):
    """The bin-tile / frame-tile paths the three recipe settings do not reach: 2, 3, 4 + 1 and 4 + 2 bin tiles of 32 per workgroup row (n_fft 64,
    128, 256, 320), a last frame tile of more and of fewer than 32 frames, a one-tile utterance.  Reference: torch.stft in float64 on the host.
    Bound, per element and rigorous for any summation order: each of re, im is a K-term f32 sum of x[n] t[n] with |t[n]| <= w[n] rounded once, so
    |re - re64| <= (K + 2) 2^-24 S with S = sum_n |x[n]| w[n]; the magnitude adds the roundings of two squares, an add and a square root."""
    from jatts_amd import features, hip
    rng = np.random.default_rng(n_fft)
    waves = [rng.standard_normal(n).astype(np.float32) for n in (101 * hop - 1, 72 * hop, n_fft // 2 + 1, 64 * hop - 1)]
    ex = features.LogMelExtractor(cuda, 16000, fft_size=n_fft, hop_size=hop, win_length=win, num_mels=20)
    rb, mag, pw = ex.stft.magnitude(features.PackedWaves.from_list(waves, cuda), True)
    assert rb.lens == [101, 73, 1 + (n_fft // 2 + 1) // hop, 64]
    nb = n_fft // 2 + 1
    assert tuple(mag.shape) == (rb.total, hip.round_up(nb, 64)) and not mag[:, nb:].any()
    w64 = torch.from_numpy(features.padded_window("hann", win, n_fft))
    u = 2.0 ** -24
    worst = 0.0
    for i, x in enumerate(waves):
        x64 = torch.from_numpy(x).double()
        ref = torch.stft(x64, n_fft, hop_length=hop, window=w64, center=True, pad_mode="reflect", return_complex=True).abs().T.numpy()
        S = (np.abs(x.astype(np.float64))[features.frame_indices(len(x), n_fft, hop)] * w64.numpy()[None, :]).sum(axis=1, keepdims=True)
        got = mag[rb.cu_host[i]:rb.cu_host[i + 1], :nb].double().cpu().numpy()
        bound = 1.5 * (n_fft + 2) * u * S + 4 * u * ref
        assert got.shape == ref.shape
        worst = max(worst, float((np.abs(got - ref) / bound).max()))
        assert (np.abs(got - ref) <= bound).all(), (i, float((np.abs(got - ref) / bound).max()))
        e64 = np.sqrt(np.maximum((ref ** 2).sum(axis=1), 1e-10))
        dp = (2 * ref * bound + bound ** 2).sum(axis=1) + (nb + 2) * u * (ref ** 2).sum(axis=1)
        e = hip.energy_frames(pw)[rb.cu_host[i]:rb.cu_host[i + 1]].double().cpu().numpy()
        assert (np.abs(e - e64) <= dp / (2 * e64) * 1.01 + 2 * u * e64).all(), i
    print(f"features[n_fft {n_fft}]: worst |error| / bound {worst:.3f}")


# ---- one wave packing, one STFT front end, one post path: every entry gives the same bits
def _three(n_fft):
    """n_fft // 2 + 1 samples (the shortest reflect padding admits), 1000 and 4097.  At n_fft 2048 reflect padding refuses 1000 samples
    (1000 <= 1024, asserted by the caller), so 2000 stand in for them there."""
    rng = np.random.default_rng(n_fft)
    return [rng.standard_normal(n).astype(np.float32) for n in (n_fft // 2 + 1, 1000 if n_fft < 2000 else 2000, 4097)]


@pytest.mark.parametrize("n_fft,hop", [(64, 7), (2048, 300)])
def test_the_three_input_forms_and_select_give_the_same_bits(cuda, n_fft, hop):
    from jatts_amd import features
    ex = features.LogMelExtractor(cuda, 16000, fft_size=n_fft, hop_size=hop, num_mels=20)
    waves = _three(n_fft)
    if n_fft == 2048:
        with pytest.raises(ValueError, match="too short to be reflect-padded"):
            ex([np.zeros(1000, dtype=np.float32)])
    pw = features.PackedWaves.from_list(waves, cuda)
    forms = [waves, [torch.from_numpy(w).to(cuda) for w in waves], pw]
    mel, feats, en = zip(*[(ex.mel(f), ex(f), ex.energy(f)) for f in forms])
    for k in (1, 2):
        assert mel[k][0].lens == mel[0][0].lens == feats[k][0].lens == [1 + len(w) // hop for w in waves]
        assert torch.equal(mel[k][1], mel[0][1]) and torch.equal(feats[k][1], feats[0][1])
        assert len(en[k]) == 3 and all(torch.equal(a, b) for a, b in zip(en[k], en[0]))
    assert feats[0][1].abs().sum() > 0 and all(e.abs().sum() > 0 for e in en[0])          # the comparison is not one of zeros
    sel, direct = pw.select([2, 0]), features.PackedWaves.from_list([waves[2], waves[0]], cuda)
    assert sel.lens == direct.lens == [4097, n_fft // 2 + 1] and sel.cu_host == direct.cu_host
    assert torch.equal(sel.x, direct.x) and torch.equal(sel.cu, direct.cu)
    rb, full = feats[0]
    rb_s, got = ex(sel)
    assert rb_s.lens == [rb.lens[2], rb.lens[0]]
    assert torch.equal(got, torch.cat([full[rb.cu_host[2]:rb.cu_host[3]], full[rb.cu_host[0]:rb.cu_host[1]]]))
    with pytest.raises(ValueError, match="no waveform"):
        features.PackedWaves.from_list([], cuda)


def test_the_three_energy_entries_give_the_same_bits(cuda):
    from jatts_amd import features
    n_fft, hop = 1024, 256
    waves = _three(n_fft)
    frames = [1 + len(w) // hop for w in waves]
    durs = [[3, 0, n - 3] for n in frames]
    en = features.Energy(fs=22050, n_fft=n_fft, hop_length=hop, use_token_averaged_energy=True, reduction_factor=1, device=cuda)
    assert getattr(en, "mel_w", None) is None and getattr(en.stft, "mel_w", None) is None         # a front end, no mel weights
    ex = features.LogMelExtractor(cuda, 22050, fft_size=n_fft, hop_size=hop)
    pw = features.PackedWaves.from_list(waves, cuda)
    ragged, by_mel = en.extract(pw, frames, durs), ex.energy(pw, frames, durs)
    for i, w in enumerate(waves):
        one = en.forward(w, frames[i], durs[i])
        assert one.dtype == np.float32 and one.shape == (3,) and one[1] == 0 and one[0] > 0
        assert torch.equal(torch.from_numpy(one), ragged[i].cpu()) and torch.equal(ragged[i], by_mel[i]), i
