"""GPU: the pitch kernels of csrc/pitch.hip against float64.

jatts_acf_from_mag is held to a float64 contraction of the same operands at every dealing branch of the framed contraction;
jatts_pitch_pick to the float64 restatement of the definition (tests/pitch_reference.py) on every frame that restatement itself decides
by more than 1e-3; jatts_f0_continuous_log + jatts_energy_adjust + jatts_token_average to the real Dio.forward (pitch_post_kat.npz);
all three to bit-identical results alone and inside a ragged batch; features.Pitch.forward and the preprocess CLI end to end."""
import csv
import os
import wave

import numpy as np
import pytest
import torch
import yaml

import pitch_reference as PR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F0MIN, F0MAX = 70, 400
# f0 of a non-fragile voiced frame against the restatement, in cents: 4 x the worst measured on an MI355X (profiles/r21_notes.md).  The
# ceiling is 1 cent: above that the kernel is wrong, not imprecise.
TOL_CENTS = 1.5e-3      # measured worst 3.762e-4 (16 kHz / 1024 / 160), 3.535e-4 (24 kHz / 2048 / 300)
POST_TOL_LOG = 8 * 2.0 ** -21      # three f32 roundings of the interpolation and a 2-ulp logf at magnitude < 8
POST_TOL_LIN = 8 * 2.0 ** -16      # the same roundings at magnitude < 256 (the tracks stay below 256 Hz) when the log is switched off


def _cents(a, b):
    return 1200.0 * np.abs(np.log2(a / b))


# ---- jatts_acf_from_mag
@pytest.mark.parametrize("K", [64, 128, 1088])
@pytest.mark.parametrize("Lp", [32, 64, 96, 160])
def test_acf_from_mag_against_float64(cuda, lib, K, Lp):
    """T in {1, 31, 33, 64, 65} as one ragged batch (frame-tile edges); Lp 32 / 64: one and two column tiles dealt pairwise, 96: three tiles,
    160: a second column workgroup.  Per element |r - ref| <= (64 + K / 64 + 2) * 2^-24 * sum_k |mag_k^2 table[k][tau]|: the two-level chain,
    the squaring and the table's rounding.  Zero table columns give exact zeros; the rows behind the last one keep their bits."""
    from jatts_amd import hip
    lens = [1, 31, 33, 64, 65]
    g = torch.Generator().manual_seed(K * 1000 + Lp)
    rows, ldm = sum(lens), K + (64 if Lp == 64 else 0)
    mag = torch.randn(rows, ldm, generator=g).abs() * torch.exp(2.0 * torch.randn(rows, 1, generator=g))
    table = torch.randn(K, Lp, generator=g) / K
    table[:, Lp - 5:] = 0.0                                   # padding columns
    table[K - 7:, :] = 0.0                                    # padding rows
    rb = hip.RaggedBatch(lens, cuda)
    guard = 3
    out = torch.full((rows + guard, Lp), -7.25, dtype=torch.float32, device=cuda)
    r = hip.acf_from_mag(rb, mag.to(cuda), table.to(cuda), out=out)
    torch.cuda.synchronize()
    got = r.cpu().numpy()
    assert np.all(got[rows:] == -7.25)                        # nothing past the last row
    got = got[:rows].astype(np.float64)
    p = mag[:, :K].double().numpy() ** 2
    t64 = table.double().numpy()
    ref, mass = p @ t64, p @ np.abs(t64)
    bound = (64 + K / 64 + 2) * U * mass
    err = np.abs(got - ref)
    print(f"K {K} Lp {Lp}: worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(err <= bound)
    assert np.all(got[:, Lp - 5:] == 0.0)


# ---- signals shared by the tests below (generated once)
def _signals(sr, specs, gate=0.05):
    return [PR.make_signal(sr, fa, fb, sec, seed=seed, gate=gate)[0] for fa, fb, sec, seed in specs]


PICK_SPECS = [(120, 300, 0.5, 11), (200, 380, 0.4, 12), (380, 200, 0.4, 13), (90, 140, 0.5, 14), (300, 395, 0.3, 15)]


@pytest.mark.parametrize("sr,n_fft,hop", [(16000, 1024, 160), (24000, 2048, 300)])
def test_pitch_pick_against_the_restatement(cuda, lib, sr, n_fft, hop):
    """Frames the float64 restatement decides by less than 1e-3 (score lead, peak against 0.45, level ratio against 0.03) are fragile and
    skipped; they must stay under 5 % of the frames.  On the rest: the same voicing, the same winning lag, f0 within TOL_CENTS."""
    from jatts_amd import features
    xs = _signals(sr, PICK_SPECS)
    ex = features.Pitch(fs=sr, n_fft=n_fft, hop_length=hop, use_token_averaged_f0=False, device=cuda)
    rb, f0, tau = ex.raw(features.PackedWaves.from_list(xs, cuda), F0MIN, F0MAX)
    f0, tau = f0.cpu().numpy().astype(np.float64), tau.cpu().numpy()
    n_frames = n_fragile = n_voiced = 0
    worst = 0.0
    for b, x in enumerate(xs):
        res = PR.analyse(x, sr, n_fft, hop, F0MIN, F0MAX)
        a, z = rb.cu_host[b], rb.cu_host[b + 1]
        assert z - a == res["f0"].size
        keep = ~res["fragile"]
        n_frames += keep.size
        n_fragile += int((~keep).sum())
        got_f0, got_tau = f0[a:z], tau[a:z]
        assert np.array_equal((got_f0 != 0)[keep], res["voiced"][keep]), (b, np.flatnonzero((got_f0 != 0) != res["voiced"]))
        k2 = keep & res["cand"]
        assert np.array_equal(got_tau[k2], res["tau"][k2]), (b, np.flatnonzero(k2 & (got_tau != res["tau"])))
        v = keep & res["voiced"]
        n_voiced += int(v.sum())
        if v.any():
            worst = max(worst, float(_cents(got_f0[v], res["f0"][v]).max()))
    print(f"sr {sr} n_fft {n_fft} hop {hop}: frames {n_frames}, fragile {n_fragile}, voiced compared {n_voiced}, worst f0 deviation {worst:.3e} cents")
    assert n_voiced > 0.4 * n_frames
    assert n_fragile <= 0.05 * n_frames
    assert worst <= TOL_CENTS


def test_batch_invariance_of_all_three_kernels(cuda, lib):
    """Every utterance alone gives the bits it gives inside a ragged batch of five -- one of a single frame, one at the L = n_fft / 2 + 1
    minimum (hop 640 > n_fft / 2 + 1 makes a single frame possible), one of more than a frame tile."""
    from jatts_amd import features, hip
    sr, n_fft, hop = 16000, 1024, 640
    lens = [600, 513, 44900, 5000, 8000]
    xs = [PR.make_signal(sr, 110 + 40 * i, 180 + 50 * i, n / sr, seed=30 + i, gate=0.004)[0][:n] for i, n in enumerate(lens)]
    assert [x.size for x in xs] == lens
    ex = features.Pitch(fs=sr, n_fft=n_fft, hop_length=hop, use_token_averaged_f0=False, device=cuda)

    def run(ws):
        pw = features.PackedWaves.from_list(ws, cuda)
        t = ex.tables(F0MIN, F0MAX)
        peak = hip.wave_gain_peak(pw.cu, len(pw.lens), pw.x, 1.0)
        rb, mag, _ = t.stft.magnitude(pw)
        r = hip.acf_from_mag(rb, mag, t.acf)
        f0, tau = hip.pitch_pick(rb, r, peak, 2, t.lo, t.hi, sr, F0MIN, t.sum_w2)
        p = hip.f0_continuous_log(rb, f0)
        return rb, [t.cpu().numpy() for t in (r, f0, tau, p)]

    rb, batch = run(xs)
    assert rb.lens == [1, 1, 71, 8, 13]
    assert (batch[1] != 0).sum() > 40                         # the comparison is not one of zeros
    for b, x in enumerate(xs):
        _, alone = run([x])
        a, z = rb.cu_host[b], rb.cu_host[b + 1]
        for name, one, many in zip(("r", "f0", "tau", "continuous log"), alone, batch):
            assert np.array_equal(one.view(np.uint32), many[a:z].view(np.uint32)), (b, name)


# ---- step 6 against the real Dio.forward
@pytest.mark.parametrize("cont,log", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_post_processing_against_the_reference(cuda, lib, golden_dir, cont, log):
    """All tracks of pitch_post_kat.npz as ONE ragged batch through jatts_f0_continuous_log, jatts_energy_adjust and jatts_token_average.
    Zeros are exactly zero; elsewhere |diff| <= POST_TOL_LOG (POST_TOL_LIN without the log)."""
    from jatts_amd import features, hip
    z = np.load(os.path.join(golden_dir, "pitch_post_kat.npz"))
    n = int(z["n"])
    tracks = [z[f"track_{i}"] for i in range(n)]
    fl = [int(z[f"feat_length_{i}"]) for i in range(n)]
    fl = [t.size if v < 0 else v for t, v in zip(tracks, fl)]
    durs = [z[f"durations_{i}"] for i in range(n)]
    rb = hip.RaggedBatch([t.size for t in tracks], cuda)
    f0 = torch.from_numpy(np.concatenate(tracks)).to(cuda)
    tol = POST_TOL_LOG if log else POST_TOL_LIN
    worst = 0.0
    for averaged, key in ((True, "out"), (False, "frames")):
        ex = features.Pitch(fs=24000, n_fft=2048, hop_length=300, use_token_averaged_f0=averaged, use_continuous_f0=bool(cont),
                            use_log_f0=bool(log), reduction_factor=1, device=cuda)
        got = ex.post(rb, f0, fl, durs if averaged else None)
        for i in range(n):
            want = z[f"{key}_{i}_{cont}{log}"]
            have = got[i].cpu().numpy()
            assert have.dtype == np.float32 and have.shape == want.shape, (key, i)
            assert np.array_equal(have == 0, want == 0), (key, i)
            d = float(np.abs(have.astype(np.float64) - want).max()) if want.size else 0.0
            worst = max(worst, d)
            assert d <= tol, (key, i, d)
    print(f"continuous {cont} log {log}: worst |diff| {worst:.3e} (bound {tol:.3e})")


# ---- end to end
E2E = dict(sr=24000, n_fft=2048, hop=300, spec=(120, 300, 0.5, 11))


def test_pitch_forward_end_to_end(cuda, lib):
    """features.Pitch.forward on one 24 kHz signal against restatement + the reference's post-processing restated.  The signal has no
    fragile frame (asserted), so every voicing decision is the restatement's; the bound is TOL_CENTS of f0, as a difference of natural
    logarithms, plus the post-processing bound."""
    from jatts_amd import features
    sr, n_fft, hop = E2E["sr"], E2E["n_fft"], E2E["hop"]
    x = _signals(sr, [E2E["spec"]])[0]
    res = PR.analyse(x, sr, n_fft, hop, F0MIN, F0MAX)
    assert not res["fragile"].any()
    t = res["f0"].size
    d = np.array([5, 0, 9, 7, 0, 11, t - 32 - 3], dtype=np.int64)
    for feat_length, dd in ((None, np.concatenate([d, [3]])), (t - 3, d), (t + 4, np.concatenate([d, [7]]))):
        want = PR.post(res["f0"], feat_length, dd)
        ex = features.Pitch(fs=sr, n_fft=n_fft, hop_length=hop, reduction_factor=1, device=cuda)
        got = ex.forward(x, F0MIN, F0MAX, feat_length, dd)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got == 0, want == 0) and (want != 0).sum() >= 5
        diff = float(np.abs(got - want).max())
        print(f"feat_length {feat_length}: worst |diff| of token-averaged log f0 {diff:.3e}")
        assert diff <= TOL_CENTS * np.log(2.0) / 1200.0 + POST_TOL_LOG
    raw = features.Pitch(fs=sr, n_fft=n_fft, hop_length=hop, use_token_averaged_f0=False, use_continuous_f0=False, use_log_f0=False, device=cuda)
    got = raw.forward(x, F0MIN, F0MAX)
    assert np.array_equal(got != 0, res["voiced"]) and got.shape == (t,)
    with pytest.raises(ValueError, match="raise f0min or fft_size"):
        raw.forward(x, 30, 400)


# ---- the CLI
CONF = dict(sampling_rate=24000, fft_size=1024, hop_size=256, win_length=None, window="hann", num_mels=80, fmin=80, fmax=7600,
            global_gain_scale=1.0, log_base=10.0, feat_list=["mel", "pitch", "energy"], pitch_extract_type="acf", energy_extract_type="energy",
            pitch_extract_f0min=90, pitch_extract_f0max=450, model_params={"reduction_factor": 1})
F0_YAML = {"spk_a": {"f0min": 80, "f0max": 400}, "spk_b": {"f0min": 100, "f0max": 500}}


def _write_toy_data(d):
    rows = []
    for i, (name, spk) in enumerate((("utt0", "spk_a"), ("utt1", "spk_b"), ("utt2", "spk_a"), ("utt3", "spk_b"))):
        x, _, _ = PR.make_signal(24000, 130 + 50 * i, 190 + 60 * i, 0.3 + 0.02 * i, seed=50 + i, gate=0.04)
        path = d / f"{name}.wav"
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(24000)
            w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        frames = 1 + x.size // CONF["hop_size"]
        rows.append({"sample_id": name, "wav_path": str(path), "spk": spk, "phonemes": "a b c d", "durations": f"4 0 9 {frames - 13}"})
    return rows


def _write_csv(path, rows):
    with open(path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0]))
        wr.writeheader()
        wr.writerows(rows)


def test_preprocess_cli_dumps_pitch(cuda, lib, tmp_path):
    """feat_list mel + pitch + energy with pitch_extract_type acf and a two-speaker f0.yaml, in this process: every dump holds a finite
    `pitch` of token count that equals Pitch.forward on the dumped wave with its speaker's range, bit for bit (the CLI groups a batch by
    range; batching changes no bits); compute_statistics writes pitch_mean / pitch_scale; the same csv with dio is refused as before."""
    from jatts_amd import features
    from jatts_amd.bin import compute_statistics, preprocess
    rows = _write_toy_data(tmp_path)
    _write_csv(tmp_path / "train.csv", rows)
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(CONF))
    (tmp_path / "f0.yaml").write_text(yaml.safe_dump(F0_YAML))
    preprocess.main(["--csv", str(tmp_path / "train.csv"), "--dumpdir", str(tmp_path / "feats"), "--config", str(tmp_path / "conf.yaml"),
                     "--f0_path", str(tmp_path / "f0.yaml"), "--batch-size", "3", "--verbose", "0"])
    with open(tmp_path / "train.csv", newline="") as f:
        out = list(csv.DictReader(f))
    assert [o["sample_id"] for o in out] == ["utt0", "utt1", "utt2", "utt3"]
    ex = features.Pitch(fs=24000, n_fft=CONF["fft_size"], hop_length=CONF["hop_size"], reduction_factor=1, device=cuda)
    for o in out:
        d = np.array([int(v) for v in o["durations"].split(" ")])
        with np.load(o["feat_path"]) as z:
            assert sorted(z.files) == ["energy", "mel", "pitch", "wave"]
            pitch, wav = z["pitch"], z["wave"]
            assert z["mel"].shape[0] == d.sum()
        rng = F0_YAML[o["spk"]]
        assert pitch.dtype == np.float32 and pitch.shape == (4,) and np.isfinite(pitch).all()
        assert pitch[1] == 0.0 and (pitch[[2, 3]] > np.log(rng["f0min"])).all() and (pitch[[2, 3]] < np.log(rng["f0max"])).all()
        want = ex.forward(wav, rng["f0min"], rng["f0max"], int(d.sum()), d)
        assert np.array_equal(pitch.view(np.uint32), want.view(np.uint32)), o["sample_id"]
    # without --f0_path the config's range applies to every speaker
    _write_csv(tmp_path / "one.csv", rows[:1])
    preprocess.main(["--csv", str(tmp_path / "one.csv"), "--dumpdir", str(tmp_path / "feats_conf"), "--config", str(tmp_path / "conf.yaml"),
                     "--verbose", "0"])
    with np.load(tmp_path / "feats_conf" / "utt0.npz") as z:
        d = np.array([int(v) for v in rows[0]["durations"].split(" ")])
        want = ex.forward(z["wave"], CONF["pitch_extract_f0min"], CONF["pitch_extract_f0max"], int(d.sum()), d)
        assert np.array_equal(z["pitch"].view(np.uint32), want.view(np.uint32))
    compute_statistics.main(["--csv", str(tmp_path / "train.csv"), "--out", str(tmp_path / "stats.npz"), "--verbose", "0"])
    with np.load(tmp_path / "stats.npz") as z:
        assert {"pitch_mean", "pitch_scale", "mel_mean", "energy_mean"} <= set(z.files)
        assert z["pitch_mean"].shape == (1,) and 4.0 < float(z["pitch_mean"][0]) < 6.5 and float(z["pitch_scale"][0]) > 0.0
    # dio is refused as before, before anything is written; so is a csv without durations
    (tmp_path / "dio.yaml").write_text(yaml.safe_dump(dict(CONF, pitch_extract_type="dio")))
    _write_csv(tmp_path / "dio.csv", rows)
    before = (tmp_path / "dio.csv").read_bytes()
    with pytest.raises(NotImplementedError, match="pyworld"):
        preprocess.main(["--csv", str(tmp_path / "dio.csv"), "--dumpdir", str(tmp_path / "dio"), "--config", str(tmp_path / "dio.yaml"),
                         "--f0_path", str(tmp_path / "f0.yaml"), "--verbose", "0"])
    assert not (tmp_path / "dio").exists() and (tmp_path / "dio.csv").read_bytes() == before
    _write_csv(tmp_path / "nodur.csv", [{k: v for k, v in r.items() if k != "durations"} for r in rows])
    with pytest.raises(ValueError, match="durations"):
        preprocess.main(["--csv", str(tmp_path / "nodur.csv"), "--dumpdir", str(tmp_path / "nodur"), "--config", str(tmp_path / "conf.yaml"),
                         "--f0_path", str(tmp_path / "f0.yaml"), "--verbose", "0"])
    assert not (tmp_path / "nodur").exists()
