"""Self-attention on the bf16x3 arithmetic (JATTS_F32E of jatts_relpos_attention; set_precision(..., attention="fp32_bf16x3") on the models).

1. the kernel against float64 over the randomised family of test_attention_fuzz_gpu.py, every case run on identical inputs as exact f32 and as F32E;
2. a sequence's F32E output alone == inside a batch; 3. the six-product code is refused; 4. the models on the real-reference bench-length goldens at the
tolerances test_benchsize_gpu.py holds "fp32_bf16x3" to; 5. the default is unchanged and B = 1 graph replay is bit-identical."""
import math
import random

import pytest
import torch

from helpers import golden_state, load_golden, maxdiff

pytestmark = pytest.mark.gpu

LENS_EDGE = [1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 257, 330]      # the tile-edge values of test_attention_fuzz_gpu.py


def _case(rng, g):
    """One random case of the family of test_attention_fuzz_gpu.one_case (f32 tensors): host inputs + the float64 attention."""
    from jatts_amd import hip
    from oracle.fs2_oracle import rel_shift_legacy
    dk = rng.choice([32, 64, 96, 128, 192, 256])
    H = rng.choice([1, 2, 4]) if dk <= 128 else rng.choice([1, 2])
    n = rng.choice([1, 2, 3, 5])
    lens = [rng.choice(LENS_EDGE) if rng.random() < 0.5 else rng.randint(1, 330) for _ in range(n)]
    rel = rng.choice(["none", "legacy", "new"])
    use_ku = rel != "none" or rng.random() < 0.5
    pad_vt = rng.random() < 0.6
    use_kv = rng.random() < 0.3
    A, R, Tm = H * dk, sum(lens), max(lens)
    q, k, v = (torch.randn(R, A, generator=g) for _ in range(3))
    ku = torch.randn(R, H, generator=g) if use_ku else None
    cap = Tm + rng.randint(0, 9)
    ldg = hip.round_up(Tm, 32) if rel == "legacy" else hip.round_up(2 * cap - 1, 32) if rel == "new" else 0
    gm = torch.randn(R, H, ldg, generator=g) if rel != "none" else None
    kv = [rng.randint(1, T) for T in lens] if use_kv else None
    scale = 1.0 / math.sqrt(dk)
    outs, o = [], 0
    for b, T in enumerate(lens):
        qs, ks, vs = (t[o:o + T].view(T, H, dk).transpose(0, 1).double() for t in (q, k, v))
        s = qs @ ks.transpose(1, 2)
        if ku is not None:
            s = s + ku[o:o + T].t().double().unsqueeze(1)
        if rel == "legacy":
            s = s + rel_shift_legacy(gm[o:o + T, :, :T].permute(1, 0, 2).double())
        elif rel == "new":          # BD'[i, j] = g[i][center - i + j], center = cap - 1
            idx = (cap - 1) - torch.arange(T)[:, None] + torch.arange(T)[None, :]
            s = s + gm[o:o + T].permute(1, 0, 2).double().gather(2, idx.expand(H, T, T))
        s = s * scale
        if kv is not None:
            s[:, :, kv[b]:] = float("-inf")
        outs.append((torch.softmax(s, -1) @ vs).transpose(0, 1).reshape(T, A))
        o += T
    return dict(dk=dk, H=H, lens=lens, rel=rel, ku=ku, pad_vt=pad_vt, kv=kv, q=q, k=k, v=v, gm=gm, ldg=ldg, cap=cap, scale=scale, ref=torch.cat(outs))


def _run(c, dev, dt, lens=None, rows=None, pad_vt=None):
    """The case (or the rows `rows` = (first, count) of it as the batch `lens`) through hip.relpos_attention with dtype code dt -> f32 output on the host."""
    from jatts_amd import hip
    lens = c["lens"] if lens is None else lens
    r0, R = (0, sum(c["lens"])) if rows is None else rows
    pad_vt = c["pad_vt"] if pad_vt is None else pad_vt
    H, dk, ldg = c["H"], c["dk"], c["ldg"]
    A = H * dk
    q, k, v = (c[n][r0:r0 + R] for n in "qkv")
    rb = hip.RaggedBatch(lens, dev)
    vcol, ldvt = rb.vt_layout() if pad_vt else (None, R)
    vt = torch.full((A, ldvt), float("nan"), dtype=torch.float32, device=dev)      # NaN in every slack column
    o = 0
    for b, T in enumerate(lens):
        c0 = int(vcol[b]) if pad_vt else o
        vt[:, c0:c0 + T] = v[o:o + T].t().to(dev)
        o += T
    gm, ku, kv = c["gm"], c["ku"], c["kv"]
    if rows is not None:
        assert kv is None
    out = hip.relpos_attention(rb, q.to(dev), A, k.to(dev), A, vt, ldvt,
                               gm[r0:r0 + R].reshape(R, H * ldg).to(dev) if gm is not None else None, ldg,
                               ku[r0:r0 + R].to(dev) if ku is not None else None, c["scale"], H, dk, dt,
                               rel_mode={"none": 0, "legacy": 1, "new": 2}[c["rel"]], rel_center=c["cap"] - 1 if c["rel"] == "new" else 0, vt_col0=vcol,
                               kv_len=torch.tensor(kv, dtype=torch.int32, device=dev) if kv is not None else None)
    assert out.dtype == torch.float32
    return out.cpu()


def _err(out, ref):
    out = out.double()
    return float((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30)) if bool(torch.isfinite(out).all()) else float("inf")


def _describe(c):
    return {k: c[k] for k in ("dk", "H", "lens", "rel", "pad_vt", "kv")} | {"ku": c["ku"] is not None}


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_emulated_attention_against_float64(cuda, lib, seed):
    """40 cases per seed, 240 in all, none left out.  e = max |out - ref| / max |ref| against the float64 attention:
    e_emul <= 5e-5 (the tolerance test_attention_fuzz_gpu.py:84 holds exact f32 to) and e_emul <= max(2 e_f32, 2^-23) (at most twice
    the exact-f32 kernel's error; 2^-23 = one f32 ulp of the normaliser, below which the output format decides the error)."""
    from jatts_amd import hip
    rng = random.Random(1000 + seed)
    g = torch.Generator().manual_seed(1000 + seed)
    rows, bad = [], []
    for i in range(40):
        c = _case(rng, g)
        e_f32, e_emul = _err(_run(c, cuda, hip.F32), c["ref"]), _err(_run(c, cuda, hip.F32E), c["ref"])
        ratio = e_emul / max(e_f32, 2.0 ** -24)
        rows.append(dict(_describe(c), e_f32=e_f32, e_emul=e_emul, ratio=ratio))
        print(f"seed {seed} case {i}: e_f32 {e_f32:.3e} e_emul {e_emul:.3e} ratio {ratio:.2f} {_describe(c)}")
        if not (e_emul <= 5e-5 and e_emul <= max(2.0 * e_f32, 2.0 ** -23)):
            bad.append(rows[-1])
    assert len(rows) == 40 and not bad, (len(bad), bad[:3])


@pytest.mark.parametrize("dk", [64, 192, 256])
def test_emulated_attention_alone_equals_inside_the_batch(cuda, lib, dk):
    from jatts_amd import hip
    rng = random.Random(dk)
    g = torch.Generator().manual_seed(dk)
    lens = {64: [65, 1, 200, 33], 192: [129, 330, 7], 256: [100, 64, 257, 31, 2]}[dk]
    for rel in ("none", "legacy", "new"):
        H, R, Tm = 2, sum(lens), max(lens)
        A = H * dk
        cap = Tm + 3
        ldg = hip.round_up(Tm, 32) if rel == "legacy" else hip.round_up(2 * cap - 1, 32) if rel == "new" else 0
        c = dict(dk=dk, H=H, lens=lens, rel=rel, pad_vt=True, kv=None, ldg=ldg, cap=cap, scale=1.0 / math.sqrt(dk),
                 q=torch.randn(R, A, generator=g), k=torch.randn(R, A, generator=g), v=torch.randn(R, A, generator=g),
                 ku=torch.randn(R, H, generator=g) if rel != "none" or rng.random() < 0.5 else None,
                 gm=torch.randn(R, H, ldg, generator=g) if rel != "none" else None)
        for pad_vt in (True, False):            # with and without vt_col0
            whole = _run(c, cuda, hip.F32E, pad_vt=pad_vt)
            assert bool(torch.isfinite(whole).all())
            o = 0
            for T in lens:
                alone = _run(c, cuda, hip.F32E, lens=[T], rows=(o, T), pad_vt=pad_vt)
                assert torch.equal(alone, whole[o:o + T]), (dk, rel, pad_vt, T)
                o += T


def test_six_product_attention_is_refused(cuda, lib):
    from jatts_amd import hip
    g = torch.Generator().manual_seed(0)
    c = dict(dk=64, H=2, lens=[40], rel="none", pad_vt=True, kv=None, ldg=0, cap=40, scale=0.125, ku=None, gm=None,
             q=torch.randn(40, 128, generator=g), k=torch.randn(40, 128, generator=g), v=torch.randn(40, 128, generator=g))
    with pytest.raises(hip._abi.JattsHipError, match="JATTS_F32E6"):
        _run(c, cuda, hip.F32E6)
    assert bool(torch.isfinite(_run(c, cuda, hip.F32E)).all())


@pytest.fixture
def route_all(monkeypatch):
    """The models' routing rule (hip.emul_attention_wins) answers from timings and may keep a head geometry -- today: all of them -- on exact f32; a model
    test under that rule would prove nothing about the emulated kernel.  These tests are about the ARITHMETIC through the models, so they force the rule
    to True and then assert that the run really launched hip.F32E."""
    from jatts_amd import hip
    monkeypatch.setattr(hip, "emul_attention_wins", lambda n_heads, d_k, rel_mode: True)


class _Recorder:
    """hip.relpos_attention wrapped: records the dtype argument of every call and calls through."""

    def __init__(self, monkeypatch):
        from jatts_amd import hip
        self.dtypes, inner = [], hip.relpos_attention

        def wrapped(*a, **k):
            self.dtypes.append(k["dtype"] if "dtype" in k else a[13])
            return inner(*a, **k)
        monkeypatch.setattr(hip, "relpos_attention", wrapped)

    def saw_emul(self):
        from jatts_amd import hip
        return hip.F32E in self.dtypes


def test_fs2_bench_utterances_with_emulated_attention(cuda, lib, monkeypatch, route_all):
    """The checks of test_benchsize_gpu.py::test_fs2_split_mode_bench_utterances_match_the_reference[fp32_bf16x3], with the attention on F32E too."""
    from jatts_amd.models import FastSpeech2
    from jatts_amd.synthetic import FS2_JSUT, pin_duration_head, synth_texts
    z, keys = load_golden("fs2_bench768.npz")
    m = FastSpeech2(idim=45, **FS2_JSUT)
    m.load_state_dict(pin_duration_head(golden_state(keys, 0), 6))
    m = m.to(cuda)
    texts = [t.to(cuda) for t in synth_texts(64, 128, 45, seed=1)]
    utts = [int(u) for u in z["utts"]]
    rec = _Recorder(monkeypatch)
    mode = dict(precision="fp32_bf16x3", attention="fp32_bf16x3")
    rb = m.set_precision(**mode).inference_batch(texts)
    assert rb["olens"] == [768] * 64
    assert rec.saw_emul(), "no relpos_attention call of the run carried hip.F32E: the routing rule sent everything to exact f32"
    for j, u in enumerate(utts):
        ref = torch.tensor(z[f"u{j}_feat_gen"])
        r1 = m.set_precision(**mode).inference_batch([texts[u]])
        rf = m.set_precision("fp32").inference_batch([texts[u]])
        assert torch.equal(r1["duration"].cpu(), torch.tensor(z[f"u{j}_duration"]))                                 # test_benchsize_gpu.py:106
        assert torch.equal(r1["feat_gen"], rb["feat_gen"][768 * u:768 * (u + 1)]), "utterance alone != inside the batch"      # :107
        es, ef = maxdiff(r1["feat_gen"], ref), maxdiff(rf["feat_gen"], ref)
        print(f"fs2 utterance {u}: emulated {es:.3e}, exact f32 {ef:.3e}")
        assert es <= 2e-3, f"bench utterance {u}: {es:.3e}"                                                         # 2e-3: test_benchsize_gpu.py:111
        assert es <= 2.0 * ef + 1e-6, f"bench utterance {u}: {es:.3e} vs exact f32 {ef:.3e} against the reference"  # 2 x + 1e-6: test_benchsize_gpu.py:112
        assert maxdiff(r1["pitch"].reshape(-1), z[f"u{j}_pitch"].reshape(-1)) <= 2e-3                               # 2e-3: test_benchsize_gpu.py:113
        assert maxdiff(r1["energy"].reshape(-1), z[f"u{j}_energy"].reshape(-1)) <= 2e-3                             # 2e-3: test_benchsize_gpu.py:114


def _seeded_noise(z):
    shape = [int(v) for v in z["noise_shape"]]
    return torch.randn(1, shape[1], shape[0], generator=torch.Generator().manual_seed(int(z["noise_seed"])))[0].t().contiguous()


def test_matcha_bench_utterance_with_emulated_attention(cuda, lib, monkeypatch, route_all):
    """The checks of test_benchsize_gpu.py::test_matcha_bench_utterance_matches_the_reference[fp32_bf16x3-0.005], with the attention on F32E too."""
    from jatts_amd.models import MatchaTTS_MAS
    from jatts_amd.synthetic import MATCHA_MAS_JSUT, matcha_golden_tweaks, pin_duration_head, synth_texts
    atol = 5e-3                                                                                                     # 5e-3: test_benchsize_gpu.py:358
    z, keys = load_golden("matcha_bench128.npz")
    m = MatchaTTS_MAS(idim=45, **MATCHA_MAS_JSUT)
    m.load_state_dict(pin_duration_head(matcha_golden_tweaks(golden_state(keys, 0)), 6))
    m = m.to(cuda).set_precision("fp32_bf16x3", attention="fp32_bf16x3")
    rec = _Recorder(monkeypatch)
    text = torch.tensor(z["u0_text"]).to(cuda)
    assert torch.equal(text.cpu(), synth_texts(64, 128, 45, seed=1)[5])
    noise = _seeded_noise(z)
    ref = z["u0_feat_gen"]
    r = m.inference_batch([text], n_timesteps=10, temperature=0.667, noise=[noise])
    assert rec.saw_emul(), "no relpos_attention call of the run carried hip.F32E: the routing rule sent everything to exact f32"
    assert torch.equal(r["duration"].cpu(), torch.tensor(z["u0_duration"])) and r["feat_gen"].shape == ref.shape == (768, 80)       # :374
    e1 = maxdiff(r["feat_gen"], ref)
    others = [t.to(cuda) for t in synth_texts(64, 128, 45, seed=1)[8:15]]
    g = torch.Generator().manual_seed(77)
    rb = m.inference_batch(others[:3] + [text] + others[3:], n_timesteps=10, temperature=0.667,
                           noise=[torch.randn(768, 80, generator=g) for _ in range(3)] + [noise] + [torch.randn(768, 80, generator=g) for _ in range(4)])
    eb = maxdiff(rb["feat_gen"][3 * 768:4 * 768], ref)
    print(f"matcha: alone {e1:.3e}, in a batch {eb:.3e}")
    assert e1 <= atol and eb <= atol, f"alone {e1:.3e}, in a batch {eb:.3e}"                                        # test_benchsize_gpu.py:382


def test_vits_bench_utterance_with_emulated_attention(cuda, lib, monkeypatch, route_all):
    """The checks of test_benchsize_gpu.py::test_vits_bench_utterance_matches_the_reference[fp32_bf16x3-0.003], with the attention on F32E too."""
    from jatts_amd.models import VITS
    from jatts_amd.synthetic import VITS_JSUT, pin_duration_head, synth_texts
    atol = 3e-3                                                                                                     # 3e-3: test_benchsize_gpu.py:385
    z, keys = load_golden("vits_bench128.npz")
    m = VITS(idim=45, spk_embed_dim=192, **VITS_JSUT)
    m.load_state_dict(pin_duration_head(golden_state(keys, 0), 6))
    m = m.to(cuda).set_precision("fp32_bf16x3", attention="fp32_bf16x3")
    rec = _Recorder(monkeypatch)
    text = torch.tensor(z["u0_text"]).to(cuda)
    spk = torch.tensor(z["u0_spemb"])
    noise = _seeded_noise(z)
    ref = z["u0_feat_gen"]
    r = m.inference_batch([text], spk.unsqueeze(0), noise=[noise])
    assert rec.saw_emul(), "no relpos_attention call of the run carried hip.F32E: the routing rule sent everything to exact f32"
    assert torch.equal(r["duration"].cpu(), torch.tensor(z["u0_duration"])) and r["feat_gen"].shape == ref.shape == (768, 80)       # :400
    e1 = maxdiff(r["feat_gen"], ref)
    others = [t.to(cuda) for t in synth_texts(64, 128, 45, seed=1)[8:15]]
    g = torch.Generator().manual_seed(78)
    spks = torch.cat([torch.randn(3, 192, generator=g), spk.unsqueeze(0), torch.randn(4, 192, generator=g)])
    rb = m.inference_batch(others[:3] + [text] + others[3:], spks,
                           noise=[torch.randn(768, 384, generator=g) for _ in range(3)] + [noise] + [torch.randn(768, 384, generator=g) for _ in range(4)])
    eb = maxdiff(rb["feat_gen"][3 * 768:4 * 768], ref)
    print(f"vits: alone {e1:.3e}, in a batch {eb:.3e}")
    assert e1 <= atol and eb <= atol, f"alone {e1:.3e}, in a batch {eb:.3e}"                                        # test_benchsize_gpu.py:409


def _fs2_small(cuda):
    from jatts_amd.models import FastSpeech2
    from jatts_amd.synthetic import FS2_SMALL
    _, keys = load_golden("fs2_small.npz")
    m = FastSpeech2(idim=20, **FS2_SMALL)
    m.load_state_dict(golden_state(keys, 0))
    return m.to(cuda)


def test_shipped_routing_rule_decides_what_the_models_launch(cuda, lib, monkeypatch):
    """Under the rule as shipped, attention="fp32_bf16x3" launches hip.F32E exactly for the runners whose head geometry the rule routes, and where it routes
    nothing the output is bit-identical to attention="fp32"."""
    from jatts_amd import hip
    m = _fs2_small(cuda)
    rec = _Recorder(monkeypatch)
    text = torch.randint(1, 20, (17,), generator=torch.Generator().manual_seed(3)).to(cuda)
    a = m.set_precision("fp32_bf16x3", attention="fp32_bf16x3").inference_batch([text])["feat_gen"].clone()
    routed = any(hip.emul_attention_wins(r.H, r.dk, 1) for r in (m._prep["enc"], m._prep["dec"]))
    assert rec.dtypes and (hip.F32E in rec.dtypes) == routed and set(rec.dtypes) <= {hip.F32, hip.F32E}
    if not routed:
        assert torch.equal(a, m.set_precision("fp32_bf16x3", attention="fp32").inference_batch([text])["feat_gen"])


def test_default_attention_is_unchanged_and_graph_replay_is_bit_identical(cuda, lib, monkeypatch, route_all):
    from jatts_amd import graphs, hip
    m = _fs2_small(cuda)
    rec = _Recorder(monkeypatch)
    text = torch.randint(1, 20, (17,), generator=torch.Generator().manual_seed(3)).to(cuda)
    a = m.set_precision("fp32_bf16x3").inference_batch([text])["feat_gen"].clone()
    b = m.set_precision("fp32_bf16x3", attention=None).inference_batch([text])["feat_gen"].clone()
    assert torch.equal(a, b)
    assert rec.dtypes and set(rec.dtypes) == {hip.F32}, "the default must keep exact-f32 attention under fp32_bf16x3"
    e = m.set_precision("fp32_bf16x3", attention="fp32").inference_batch([text])["feat_gen"].clone()
    assert torch.equal(a, e)
    # B = 1 drop-in path with the emulated attention: eager launches, then first sight eager, second captured, third replayed
    m.set_precision("fp32_bf16x3", attention="fp32_bf16x3")
    on, graphs.ENABLED = graphs.ENABLED, False
    try:
        ref = m.inference(text)
        ref = {k: v.clone() for k, v in ref.items()}
    finally:
        graphs.ENABLED = on
    assert hip.F32E in rec.dtypes
    got = [m.inference(text) for _ in range(3)]
    gc = m._prep["graphs"]
    assert gc.stats["captured"] >= 1 and gc.stats["replayed"] >= 1 and gc.stats["failed"] == 0, gc.stats
    for o in got:
        for k in o:
            assert torch.equal(ref[k], o[k]), f"{k}: graph replay with the emulated attention differs from the eager launches"
