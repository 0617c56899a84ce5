"""GPU: the resident dataset and the batch loader (jatts_amd/data.py) against a host restatement of TTSDataset + FastSpeech2Collater on a toy
corpus of 7 utterances, bit for bit; and against one batch of the REAL collater over REAL StandardScaler output (tests/golden/collate_kat.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from toy_corpus import GEOM, TOKEN_LIST, expected_batch, write_corpus, write_csv

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.int64: torch.int64}[t.dtype])


def assert_batch_equal(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        g = got[k]
        if w is None:
            assert g is None, k
            continue
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.is_cuda == (not k.endswith("lens")), k         # features on the device, length vectors on the host
        assert torch.equal(bits(g.cpu()), bits(w)), k


def dataset(corpus, feat_list, cuda, **kw):
    from jatts_amd.data import ResidentDataset
    return ResidentDataset(corpus["csv"], corpus["stats"], list(feat_list), corpus["tokens"], "phonemes", device=cuda, **kw)


@pytest.mark.parametrize("feat_list,durations,odim", [(("mel", "pitch", "energy"), True, 80), (("mel", "spkemb"), True, 5), (("mel",), False, 6)])
def test_every_batch_of_an_epoch_equals_the_host_restatement(cuda, tmp_path, feat_list, durations, odim):
    """Train loader: batch ids equal BatchSampler(RandomSampler(...), 3, False)'s under the same torch seed, the short last batch is kept, an
    epoch visits every utterance once; dev loader: sequential.  mel dim 80 (16-byte rows), 5 and 6 (rows off 16 bytes)."""
    from torch.utils.data import BatchSampler, RandomSampler
    from jatts_amd.data import BatchLoader
    corpus = write_corpus(tmp_path, feat_list, durations, odim=odim)
    ds = dataset(corpus, feat_list, cuda)
    assert len(ds) == len(GEOM) == 7
    loader = BatchLoader(ds, 3, shuffle=True)
    assert len(loader) == 3
    for seed in (0, 5):
        torch.manual_seed(seed)
        want_ids = list(BatchSampler(RandomSampler(range(7)), 3, False))
        torch.manual_seed(seed)
        seen = []
        for ids, batch in zip(want_ids, loader):
            assert_batch_equal(batch, expected_batch(corpus, ids, feat_list, durations))
            seen += ids
        assert [len(b) for b in want_ids] == [3, 3, 1] and sorted(seen) == list(range(7))
    dev = BatchLoader(ds, 3, shuffle=False)
    for n, batch in enumerate(dev):
        assert_batch_equal(batch, expected_batch(corpus, list(range(7))[3 * n:3 * n + 3], feat_list, durations))
    assert n == 2
    a = [b["ilens"].tolist() for b in BatchLoader(ds, 3, shuffle=True, seed=11)]
    assert a == [b["ilens"].tolist() for b in BatchLoader(ds, 3, shuffle=True, seed=11)]       # a seeded loader has a generator of its own
    if "durations" in batch:
        assert batch["duration_lens"] is batch["durations_lens"] or torch.equal(batch["duration_lens"], batch["durations_lens"])


def test_batch_equals_the_real_collater_on_real_scaler_output(cuda, tmp_path, golden_dir):
    from jatts_amd.data import BatchLoader, ResidentDataset
    z = np.load(os.path.join(golden_dir, "collate_kat.npz"))
    toks = ["<blank>", "<unk>"] + [f"p{i}" for i in range(2, 10)]
    rows = []
    for n in range(3):
        path = str(tmp_path / f"u{n}.npz")
        np.savez(path, **{k: z[f"raw_{k}_{n}"] for k in ("mel", "pitch", "energy", "spkemb")})
        rows.append({"sample_id": f"u{n}", "feat_path": path, "phonemes": " ".join(toks[int(i)] for i in z[f"tokens_{n}"]),
                     "durations": " ".join(str(int(d)) for d in z[f"durations_{n}"])})
    write_csv(str(tmp_path / "kat.csv"), rows)
    (tmp_path / "tokens.txt").write_text("".join(t + "\n" for t in toks), encoding="utf-8")
    np.savez(str(tmp_path / "stats.npz"), **{k: z[k] for k in z.files if k.endswith("_mean") or k.endswith("_scale")})
    ds = ResidentDataset(str(tmp_path / "kat.csv"), str(tmp_path / "stats.npz"), ["mel", "pitch", "energy", "spkemb"], str(tmp_path / "tokens.txt"),
                         "phonemes", device=cuda)
    batch, = list(BatchLoader(ds, 3, shuffle=False))
    keys = json.loads(str(z["batch_keys"]))
    assert set(batch) == {k for k, _, _ in keys} | {"duration_lens"}          # the key the reference's trainers read, next to the collater's
    for k, dtype, shape in keys:
        w = torch.from_numpy(z[f"batch_{k}"])
        assert str(batch[k].dtype) == dtype and list(batch[k].shape) == shape, k
        assert torch.equal(bits(batch[k].cpu()), bits(w)), k
    assert torch.equal(batch["duration_lens"], batch["durations_lens"])


def test_unknown_token_maps_to_unk(cuda, tmp_path):
    from jatts_amd.data import BatchLoader
    corpus = write_corpus(tmp_path, ("mel",), False, odim=4)
    rows = corpus["rows"]
    first = rows[0]["phonemes"].split(" ")
    rows[0]["phonemes"] = " ".join(["zz"] + first[1:])
    write_csv(corpus["csv"], rows)
    batch = next(iter(BatchLoader(dataset(corpus, ("mel",), cuda), 2, shuffle=False)))
    assert batch["xs"][0, 0].item() == TOKEN_LIST.index("<unk>") and batch["xs"][0, 1].item() == TOKEN_LIST.index(first[1])


def test_load_time_refusals_name_the_utterance_or_the_limit(cuda, tmp_path):
    feat_list = ("mel", "pitch", "energy")

    def broken(sub, edit, feats=feat_list, **kw):
        corpus = write_corpus(tmp_path / sub, feats, True, odim=4)
        rows = corpus["rows"]
        edit(rows, corpus)
        write_csv(corpus["csv"], rows)
        return corpus, kw

    def resave(row, **changes):
        with np.load(row["feat_path"]) as z:
            d = {k: z[k] for k in z.files}
        for k, v in changes.items():
            if v is None:
                del d[k]
            else:
                d[k] = v
        np.savez(row["feat_path"], **d)

    cases = {
        "missing": (lambda rows, c: resave(rows[2], energy=None), "utt2"),
        "n_durations": (lambda rows, c: rows[3].update(durations=rows[3]["durations"] + " 1"), "utt3"),
        "sum_durations": (lambda rows, c: rows[5].update(durations=" ".join(["1"] * 6)), "utt5"),
        "pitch_rows": (lambda rows, c: resave(rows[0], pitch=np.zeros(4, np.float32)), "utt0"),
        "energy_rows": (lambda rows, c: resave(rows[6], energy=np.zeros(1, np.float32)), "utt6"),
        "empty_tokens": (lambda rows, c: rows[4].update(phonemes=" "), "utt4"),
        "empty_mel": (lambda rows, c: (resave(rows[1], mel=np.zeros((0, 4), np.float32)), rows[1].update(durations="0")), "utt1"),
    }
    for sub, (edit, sid) in cases.items():
        corpus, _ = broken(sub, edit)
        with pytest.raises(ValueError, match=sid):
            dataset(corpus, feat_list, cuda)
    corpus = write_corpus(tmp_path / "ok", feat_list, True, odim=4)
    with pytest.raises(ValueError, match="resident_gb"):
        dataset(corpus, feat_list, cuda, resident_gb=1e-7)
    with pytest.raises(ValueError, match="encodec"):
        dataset(corpus, ("mel", "encodec_24khz"), cuda)
    with pytest.raises(ValueError, match="prompt_strategy"):
        dataset(corpus, feat_list, cuda, prompt_strategy="given")
