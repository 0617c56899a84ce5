"""The B = 1 drop-in path by hipGraph replay (jatts_amd/graphs.py; reference call sites jatts/bin/tts_decode.py:230,249): `model.inference(x)` and
`vocoder.decode(mel)` answered from a captured graph are BIT-IDENTICAL to the eager launches -- same kernels, same order, same arithmetic -- for
every arithmetic, for new inputs of a captured signature, and the tensors handed out are not overwritten by the next replay."""
import pytest
import torch

from helpers import golden_state, load_golden, maxdiff
from jatts_amd.synthetic import FS2_SMALL, HIFIGAN_V1_22K, HIFIGAN_V1_24K, synth_hifigan_state

pytestmark = pytest.mark.gpu


def _eager(fn):
    from jatts_amd import graphs
    on, graphs.ENABLED = graphs.ENABLED, False
    try:
        return fn()
    finally:
        graphs.ENABLED = on


def _fs2(cuda, prec, **kw):
    from jatts_amd.models import FastSpeech2
    _, keys = load_golden("fs2_small.npz")
    m = FastSpeech2(idim=20, **FS2_SMALL, **kw)
    if kw:
        from jatts_amd.synthetic import synth_state_dict
        m.load_state_dict(synth_state_dict(m.state_dict(), 0))
    else:
        m.load_state_dict(golden_state(keys, 0))
    return m.to(cuda).set_precision(prec)


@pytest.mark.parametrize("prec", ["fp32", "fp32_bf16x3", "fp32_bf16x3_6p", "fp32_split", "fp16"])
def test_fs2_inference_graph_is_bit_identical(cuda, lib, prec):
    m = _fs2(cuda, prec)
    g = torch.Generator().manual_seed(3)
    texts = [torch.randint(1, 20, (17,), generator=g).to(cuda) for _ in range(5)] + [torch.randint(1, 20, (9,), generator=g).to(cuda) for _ in range(3)]
    ref = _eager(lambda: [m.inference(t) for t in texts])
    got = [m.inference(t) for t in texts]          # 17 phonemes: eager, capture, replay x3; 9 phonemes: eager, capture, replay
    gc = m._prep["graphs"]
    assert gc.stats["captured"] >= 2 and gc.stats["replayed"] >= 3 and gc.stats["failed"] == 0, gc.stats
    for r, o in zip(ref, got):
        assert set(o) == {"feat_gen", "duration", "pitch", "energy"}
        for k in o:
            assert torch.equal(r[k], o[k]), f"{prec} {k}: replay differs from the eager launches"
    # the tensors of an earlier call survive later replays of the same graph
    keep = m.inference(texts[0])
    snap = {k: v.clone() for k, v in keep.items()}
    m.inference(texts[1])
    m.inference(texts[2])
    for k in keep:
        assert torch.equal(keep[k], snap[k])
    assert torch.equal(keep["feat_gen"], ref[0]["feat_gen"])


def test_fs2_graph_with_speaker_embedding_alpha_and_durations(cuda, lib):
    m = _fs2(cuda, "fp32", spk_embed_dim=16, spk_embed_integration_type="concat")
    g = torch.Generator().manual_seed(5)
    text = [torch.randint(1, 20, (13,), generator=g).to(cuda) for _ in range(4)]
    spk = [torch.randn(16, generator=g).to(cuda) for _ in range(4)]
    for alpha in (1.0, 1.3):
        ref = _eager(lambda: [m.inference(t, spembs=s, alpha=alpha) for t, s in zip(text, spk)])
        got = [m.inference(t, spembs=s, alpha=alpha) for t, s in zip(text, spk)]
        for r, o in zip(ref, got):
            assert torch.equal(r["feat_gen"], o["feat_gen"]) and torch.equal(r["duration"], o["duration"])
    # teacher-forced durations through inference_batch (B = 1): its own signature
    d = torch.full((13,), 3, dtype=torch.int64)
    ref = _eager(lambda: [m.inference_batch([t], spembs=s.unsqueeze(0), durations=[d])["feat_gen"] for t, s in zip(text, spk)])
    got = [m.inference_batch([t], spembs=s.unsqueeze(0), durations=[d])["feat_gen"] for t, s in zip(text, spk)]
    for r, o in zip(ref, got):
        assert torch.equal(r, o)
    assert m._prep["graphs"].stats["failed"] == 0


def test_bad_token_id_still_raises_under_replay(cuda, lib):
    m = _fs2(cuda, "fp32")
    t = torch.randint(1, 20, (11,), generator=torch.Generator().manual_seed(1)).to(cuda)
    for _ in range(3):
        m.inference(t)
    bad = t.clone()
    bad[4] = 20
    with pytest.raises(IndexError):
        m.inference(bad)
    m.inference(t)        # and the counter was reset: the next good utterance passes


@pytest.mark.parametrize("prec", ["fp32", "fp32_bf16x3", "fp16"])
@pytest.mark.parametrize("params", [HIFIGAN_V1_22K, HIFIGAN_V1_24K], ids=["22k", "24k"])
def test_vocoder_decode_graph_is_bit_identical(cuda, lib, prec, params):
    from jatts_amd.vocoder import Vocoder
    p = dict(params, channels=128)
    sd = synth_hifigan_state(p, seed=0)
    g = torch.Generator().manual_seed(2)
    mean, scale = torch.randn(80, generator=g).tolist(), (torch.rand(80, generator=g) + 0.5).tolist()
    v = Vocoder(sd, {"sampling_rate": 24000, "generator_type": "HiFiGANGenerator", "generator_params": p}, {"mean": mean, "scale": scale}, cuda,
                trg_stats={"mean": [0.1] * 80, "scale": [1.1] * 80}).set_precision(prec)
    mels = [torch.randn(23, 80, generator=g).to(cuda) for _ in range(4)] + [torch.randn(40, 80, generator=g).to(cuda) for _ in range(3)]
    ref = _eager(lambda: [v.decode(c)[0] for c in mels])
    got = [v.decode(c)[0] for c in mels]
    gc = v.model._prep["graphs"]
    assert gc.stats["captured"] == 2 and gc.stats["replayed"] == 3 and gc.stats["failed"] == 0, gc.stats
    for c, r, o in zip(mels, ref, got):
        assert o.shape == r.shape and o.numel() == c.shape[0] * v.model.hop
        assert torch.equal(r, o), f"{prec}: replayed waveform differs from the eager launches"
    keep = v.decode(mels[0])[0]
    snap = keep.clone()
    v.decode(mels[1])
    assert torch.equal(keep, snap) and torch.equal(keep, ref[0])


def test_graph_cache_evicts_least_recently_used(cuda, lib):
    from jatts_amd.graphs import GraphCache
    gc = GraphCache(max_graphs=2)
    x = torch.arange(8, dtype=torch.float32, device=cuda)
    for key in ("a", "b", "c", "a"):
        for _ in range(3):
            y = gc.run(key, lambda t: t * 2 + 1, (x,))
            assert torch.equal(y, x * 2 + 1)
    assert len(gc) == 2 and gc.stats["captured"] == 4      # "a" was evicted by "c" and captured again


def test_graph_cache_answers_a_failed_capture_eagerly_and_never_retries(cuda, lib):
    """An exception leaving the capture: the call is answered by eager launches, the signature stays eager-only, nothing stays pinned
    (hip._KEEP), and other signatures capture and replay as ever."""
    from jatts_amd import hip
    from jatts_amd.graphs import GraphCache
    gc = GraphCache(max_graphs=2)
    x = torch.arange(8, dtype=torch.float32, device=cuda)

    def fn(t):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("not under capture")
        return t * 2 + 1
    for _ in range(3):
        assert torch.equal(gc.run("a", fn, (x,)), x * 2 + 1)
    assert gc.stats["failed"] == 1 and gc.stats["captured"] == 0 and gc._g["a"].get("eager_only") and len(gc) == 0
    assert hip._KEEP[0] is None
    for _ in range(3):
        assert torch.equal(gc.run("b", lambda t: t * 2 + 1, (x,)), x * 2 + 1)
    assert gc.stats == dict(eager=3, captured=1, replayed=1, failed=1) and len(gc) == 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# Replay after the process has done other work: the bounded upload caches evict, the conformer stacks' positional tables regrow.


def _vocoder(cuda, prec, params):
    from jatts_amd.vocoder import Vocoder
    p = dict(params, channels=128)
    g = torch.Generator().manual_seed(4)
    stats = {"mean": torch.randn(80, generator=g).tolist(), "scale": (torch.rand(80, generator=g) + 0.5).tolist()}
    trg = {"mean": [0.1] * 80, "scale": [1.1] * 80}
    v = Vocoder(synth_hifigan_state(p, seed=0), {"sampling_rate": 24000, "generator_type": "HiFiGANGenerator", "generator_params": p}, stats,
                cuda, trg_stats=trg).set_precision(prec)
    return v, p, stats, trg


def _watch_captures(monkeypatch):
    """-> a list that gets one (keep list, geometry tensors) pair per capture: the list hip.keep_begin hands the GraphCache, and every
    RaggedBatch.cu whose address a launch recorded into the graph (RaggedBatch.struct, and the length regulator's output offsets)."""
    from jatts_amd import hip
    caps = []
    begin, struct, lr_gather = hip.keep_begin, hip.RaggedBatch.struct, hip.lr_gather

    def keep_begin():
        lst = begin()
        caps.append((lst, []))
        return lst

    def logged_struct(self, len_mul=1):
        if torch.cuda.is_current_stream_capturing():
            caps[-1][1].append(self.cu)
        return struct(self, len_mul)

    def logged_lr_gather(rb, cum, rb_out, *a, **k):
        if torch.cuda.is_current_stream_capturing():
            caps[-1][1].append(rb_out.cu)
        return lr_gather(rb, cum, rb_out, *a, **k)

    monkeypatch.setattr(hip, "keep_begin", keep_begin)
    monkeypatch.setattr(hip.RaggedBatch, "struct", logged_struct)
    monkeypatch.setattr(hip, "lr_gather", logged_lr_gather)
    return caps


def _assert_geometry_pinned(caps, caches, n_captures):
    """Every geometry a captured graph reads must be referenced, by identity, from the record of that graph in its GraphCache: the
    upload caches evict and free their tensors, and a replay reads whatever then lives at the recorded address."""
    assert len(caps) == n_captures, (len(caps), n_captures)
    states = [st for gc in caches for st in gc._g.values() if st.get("graph") is not None]
    for keep, seen in caps:
        assert seen, "no ragged geometry was recorded during a capture"
        owner = [st for st in states if st.get("keep") is keep]
        assert len(owner) == 1, "the capture's keep list is not held by a graph record"
        pinned = [t for t in owner[0]["keep"] if torch.is_tensor(t)]
        loose = [t for t in seen if not any(t is p for p in pinned)]
        assert not loose, f"{len(loose)} of {len(seen)} geometry tensors read by the graph are not pinned by it (cu {sorted({tuple(t.tolist()) for t in loose})})"


@pytest.mark.parametrize("prec", ["fp32", "fp32_bf16x3"])
@pytest.mark.parametrize("case", ["plain", "spembs_alpha", "sids", "durations", "voc22k", "voc24k"])
def test_captured_graph_pins_the_geometry_it_reads(cuda, lib, monkeypatch, prec, case):
    """Structural: a signature's second sight captures; every RaggedBatch.cu baked into that graph must be in the graph's own record
    (st["keep"]), so no cache eviction can free it while the graph lives.  Nothing is replayed over freed memory here."""
    caps = _watch_captures(monkeypatch)
    g = torch.Generator().manual_seed(9)
    if case.startswith("voc"):
        v, *_ = _vocoder(cuda, prec, HIFIGAN_V1_22K if case == "voc22k" else HIFIGAN_V1_24K)
        for _ in range(2):
            v.decode(torch.randn(27, 80, generator=g).to(cuda))
        caches = [v.model._prep["graphs"]]
        n = 1
    else:
        kw = {"spembs_alpha": dict(spk_embed_dim=16, spk_embed_integration_type="concat"), "sids": dict(spks=4)}.get(case, {})
        m = _fs2(cuda, prec, **kw)
        t = torch.randint(1, 20, (14,), generator=g).to(cuda)        # the same utterance twice: its predicted T_feats keys the back half
        s = torch.randn(16, generator=g).to(cuda)
        for _ in range(2):
            if case == "plain":
                m.inference(t)
            elif case == "spembs_alpha":
                m.inference(t, spembs=s, alpha=1.3)
            elif case == "sids":
                m.inference(t, sids=torch.tensor([2]).to(cuda))
            else:
                m.inference_batch([t], durations=[torch.full((14,), 2, dtype=torch.int64)])
        caches = [m._prep["graphs"]]
        n = 2
    assert caches[0].stats["captured"] == n and caches[0].stats["failed"] == 0, caches[0].stats
    _assert_geometry_pinned(caps, caches, n)


def test_graph_replay_survives_upload_cache_churn(cuda, lib, monkeypatch):
    """The stream of a long decode run: after the graphs were captured, hundreds of other geometries pass through the bounded caches, which
    evict and free the tensors they held.  Replays must still equal the eager launches bit for bit.  The freed small blocks are refilled with
    zeros before the replays, so a graph that read a freed geometry would see zero-length sequences (no out-of-bounds access) and fail the
    comparison.  The structural check runs first: nothing is churned under a graph that does not pin its geometry."""
    import gc as pygc

    from jatts_amd import hip
    caps = _watch_captures(monkeypatch)
    m = _fs2(cuda, "fp32")
    v, *_ = _vocoder(cuda, "fp32", HIFIGAN_V1_22K)
    g = torch.Generator().manual_seed(11)
    d = torch.randint(1, 4, (15,), generator=g)
    texts = [torch.randint(1, 20, (15,), generator=g).to(cuda) for _ in range(5)]
    mels = [torch.randn(31, 80, generator=g).to(cuda) for _ in range(5)]
    for i in range(2):                                   # first sight eager, second captures
        m.inference_batch([texts[i]], durations=[d])
        v.decode(mels[i])
    fgc, vgc = m._prep["graphs"], v.model._prep["graphs"]
    assert fgc.stats["captured"] == 2 and vgc.stats["captured"] == 1
    _assert_geometry_pinned(caps, [fgc, vgc], 3)
    ref_f = _eager(lambda: [m.inference_batch([t], durations=[d])["feat_gen"] for t in texts[2:]])
    ref_v = _eager(lambda: [v.decode(c)[0] for c in mels[2:]])
    (geometry,) = [c for c in hip.device_caches() if c.name == "RaggedBatch geometry"]
    for n in range(3 * geometry.max_entries // 2):       # fresh geometries: the oldest entries are evicted
        hip.RaggedBatch([100003 + n], cuda)
    assert len(geometry) == geometry.max_entries
    hip.clear_device_caches()
    pygc.collect()
    torch.cuda.synchronize()
    fill = [torch.zeros(128, dtype=torch.int32, device=cuda) for _ in range(8192)]    # 512-byte blocks: the size class of a freed geometry
    torch.cuda.synchronize()
    rf, rv = fgc.stats["replayed"], vgc.stats["replayed"]
    got_f = [m.inference_batch([t], durations=[d])["feat_gen"] for t in texts[2:]]
    got_v = [v.decode(c)[0] for c in mels[2:]]
    assert fgc.stats["replayed"] == rf + 2 * len(got_f) and vgc.stats["replayed"] == rv + len(got_v), (fgc.stats, vgc.stats)
    for r, o in zip(ref_f + ref_v, got_f + got_v):
        assert torch.equal(r, o), "a replay after cache churn differs from the eager launches"
    del fill


@pytest.mark.parametrize("prec", ["fp32", "fp32_bf16x3"])
def test_positional_table_regrowth_eager_and_graph_match_the_reference(cuda, lib, prec):
    """The reference's LegacyRelPositionalEncoding regrows its table for good when it first sees more than 5000 positions, which changes the
    table's values for every later short utterance (fs2_pe_regrow_small.npz: short call, > 5000-frame teacher-forced call, short call on ONE
    reference object).  Eager: the same three calls match both answers.  Graph: signatures captured before the regrowth must not answer after
    it -- the later calls equal the eager post-regrowth launches bit for bit and match the reference's second answer."""
    from jatts_amd.models import FastSpeech2
    from jatts_amd.models._conformer import PE_TABLE_LEN
    z, keys = load_golden("fs2_pe_regrow_small.npz")
    t = lambda k: torch.tensor(z[k])  # noqa: E731
    T_long = int(z["long_t_feats"])

    def model():
        m = FastSpeech2(idim=20, **FS2_SMALL)
        m.load_state_dict(golden_state(keys, 0))
        return m.to(cuda).set_precision(prec)

    u = t("u_text").to(cuda)
    long_text = t("long_text").to(cuda)

    def long_call(m):
        r = m.inference(long_text, durations=t("long_durations"), pitch=t("long_pitch"), energy=t("long_energy"), use_teacher_forcing=True)
        assert r["feat_gen"].shape[0] == T_long
        assert m._prep["dec"].pe_len == T_long and m._prep["enc"].pe_len == PE_TABLE_LEN

    def check(r, p):
        assert torch.equal(r["duration"].cpu(), t(f"{p}_duration"))
        for k in ("feat_gen", "pitch", "energy"):
            assert maxdiff(r[k], z[f"{p}_{k}"]) <= 2e-3, (prec, p, k, maxdiff(r[k], z[f"{p}_{k}"]))

    me = model()
    eager_a = _eager(lambda: me.inference(u))
    _eager(lambda: long_call(me))
    eager_b = _eager(lambda: me.inference(u))
    check(eager_a, "a")
    check(eager_b, "b")

    mg = model()
    pre = [mg.inference(u) for _ in range(2)]            # eager, capture (front and back)
    gc = mg._prep["graphs"]
    assert gc.stats["captured"] == 2
    long_call(mg)
    post = [mg.inference(u) for _ in range(3)]
    assert gc.stats["failed"] == 0 and gc.stats["replayed"] >= 2, gc.stats
    for o in pre:
        for k in o:
            assert torch.equal(o[k], eager_a[k]), k
    for i, o in enumerate(post):
        for k in o:
            assert torch.equal(o[k], eager_b[k]), f"{prec}: call {i} after the regrowth: {k} differs from the eager post-regrowth launches"
        check(o, "b")


@pytest.mark.parametrize("prec", ["fp32", "fp32_bf16x3"])
def test_decode_stream_with_small_graph_caches_matches_eager_and_the_oracles(cuda, lib, prec):
    """A decode loop over a test set: 40 B = 1 utterances of 15 distinct lengths, some texts repeated, text -> mel -> waveform, with room for
    only three graphs per model, so captures, replays and least-recently-used evictions interleave while earlier outputs are kept.  Every
    call equals the eager launches bit for bit and the fp32 oracles within the suite's bounds (mel 2e-3, waveform 2e-4)."""
    from jatts_amd.graphs import GraphCache
    from oracle.fs2_oracle import fs2_inference
    from oracle.hifigan_oracle import hifigan_generate, vocoder_normalize
    _, keys = load_golden("fs2_small.npz")
    sd = golden_state(keys, 0)
    m = _fs2(cuda, prec)
    m._prepare()["graphs"] = GraphCache(max_graphs=3)
    v, p, stats, trg = _vocoder(cuda, prec, HIFIGAN_V1_22K)
    v.model._prepare()["graphs"] = GraphCache(max_graphs=3)
    vsd = synth_hifigan_state(p, seed=0)
    g = torch.Generator().manual_seed(21)
    lengths = list(range(4, 19))
    pool = {n: [] for n in lengths}
    calls = []
    for i in range(40):
        n = lengths[int(torch.randint(len(lengths), (1,), generator=g))] if i >= 2 else lengths[0]
        if pool[n] and int(torch.randint(2, (1,), generator=g)):
            text = pool[n][int(torch.randint(len(pool[n]), (1,), generator=g))]
        else:
            text = torch.randint(1, 20, (n,), generator=g)
            pool[n].append(text)
        calls.append(text)
    outs = []
    for text in calls:
        r = m.inference(text.to(cuda))
        outs.append((r, v.decode(r["feat_gen"])[0]))
    fgc, vgc = m._prep["graphs"], v.model._prep["graphs"]
    for gc, per_call in ((fgc, 2), (vgc, 1)):
        s = gc.stats
        assert s["failed"] == 0 and s["captured"] + s["replayed"] + s["eager"] == per_call * len(calls), s
        assert s["captured"] > 3 and s["replayed"] > 0 and len(gc) <= 3, s     # more captures than room: evictions happened
    oracle = {}
    for text, (r, y) in zip(calls, outs):
        e = _eager(lambda: m.inference(text.to(cuda)))
        for k in r:
            assert torch.equal(r[k], e[k]), f"{prec} T_text {len(text)}: {k} differs from the eager launches"
        assert torch.equal(y, _eager(lambda: v.decode(r["feat_gen"])[0]))
        key = tuple(text.tolist())
        if key not in oracle:
            oracle[key] = fs2_inference(sd, text, 2)
        o = oracle[key]
        assert torch.equal(r["duration"].cpu(), o["duration"])
        assert maxdiff(r["feat_gen"], o["feat_gen"]) <= 2e-3, (prec, len(text), maxdiff(r["feat_gen"], o["feat_gen"]))
        mel = r["feat_gen"].cpu()
        c = vocoder_normalize(mel, torch.tensor(trg["mean"]), torch.tensor(trg["scale"]), torch.tensor(stats["mean"]), torch.tensor(stats["scale"]))
        ref = hifigan_generate(vsd, c, p["upsample_scales"], p["resblock_dilations"])
        assert y.shape == ref.shape and maxdiff(y, ref) <= 2e-4, (prec, mel.shape[0], maxdiff(y, ref))
