"""A toy training corpus written with numpy (no stage-1 run): .npz dumps, a stats .npz, a token list and csv files, plus the host restatement
of what a batch must hold (tts_dataset.py:108-145 + collaters/fastspeech2.py:17-107).  Shared by the stage-3 tests."""
import csv
import os

import numpy as np

GEOM = [(3, 7), (1, 1), (5, 12), (4, 9), (2, 2), (6, 16), (3, 5)]      # (tokens, frames) of the 7 utterances
SYMBOLS = ["a", "i", "u", "e", "o", "k", "s", "t", "n", "pau"]
TOKEN_LIST = ["<blank>", "<unk>"] + SYMBOLS + ["<sos/eos>"]


def write_corpus(root, feat_list=("mel", "pitch", "energy"), durations=True, odim=80, sdim=16, geom=GEOM, seed=0, name="train"):
    """-> dict(csv, stats, tokens, items): ``items[n]`` holds the raw arrays, token ids and durations of utterance n."""
    root = str(root)
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "dump", name), exist_ok=True)
    dims = {"mel": odim, "pitch": 1, "energy": 1, "spkemb": sdim}
    stats = {}
    srng = np.random.default_rng(99)
    for k in ("mel", "pitch", "energy", "spkemb"):
        stats[f"{k}_mean"] = srng.normal(0.0, 1.0, dims[k]).astype(np.float32)
        stats[f"{k}_scale"] = srng.uniform(0.5, 2.0, dims[k]).astype(np.float32)
    stats_path = os.path.join(root, "stats.npz")
    np.savez(stats_path, **stats)
    tokens_path = os.path.join(root, "tokens.txt")
    with open(tokens_path, "w", encoding="utf-8") as f:
        f.write("".join(t + "\n" for t in TOKEN_LIST))
    items, rows = [], []
    for n, (nt, nf) in enumerate(geom):
        cuts = np.sort(rng.choice(np.arange(1, nf), nt - 1, replace=False)) if nt > 1 else np.array([], dtype=np.int64)
        dur = np.diff(np.concatenate([[0], cuts, [nf]])).astype(np.int64)
        phn = [SYMBOLS[int(i)] for i in rng.integers(0, len(SYMBOLS), nt)]
        raw = {"mel": rng.normal(0.0, 1.5, (nf, odim)).astype(np.float32), "pitch": rng.normal(0.0, 1.0, nt).astype(np.float32),
               "energy": rng.normal(0.0, 1.0, nt).astype(np.float32), "spkemb": rng.normal(0.0, 1.0, sdim).astype(np.float32)}
        path = os.path.join(root, "dump", name, f"utt{n}.npz")
        np.savez(path, **{k: raw[k] for k in feat_list})
        row = {"sample_id": f"utt{n}", "feat_path": path, "phonemes": " ".join(phn)}
        if durations:
            row["durations"] = " ".join(str(int(d)) for d in dur)
        rows.append(row)
        items.append({"raw": raw, "ids": np.asarray([TOKEN_LIST.index(p) for p in phn], dtype=np.int64), "dur": dur, "row": row})
    csv_path = os.path.join(root, f"{name}.csv")
    write_csv(csv_path, rows)
    return {"csv": csv_path, "stats": stats_path, "tokens": tokens_path, "items": items, "stats_arrays": stats, "rows": rows}


def write_csv(path, rows):
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0]))
        w.writeheader()
        w.writerows(rows)


def normalised(corpus, n, name):
    x = corpus["items"][n]["raw"][name]
    x = x.reshape(1, -1) if name == "spkemb" else x.reshape(-1, 1) if name in ("pitch", "energy") else x
    return (x - corpus["stats_arrays"][f"{name}_mean"]) / corpus["stats_arrays"][f"{name}_scale"]      # float32, one subtract, one divide


def pad(arrays):
    out = np.zeros((len(arrays), max(a.shape[0] for a in arrays)) + arrays[0].shape[1:], dtype=arrays[0].dtype)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return out


def expected_batch(corpus, ids, feat_list, durations=True):
    """The collater's dict for the utterances ``ids`` as numpy arrays (None for an absent spkembs)."""
    it = corpus["items"]
    out = {"xs": pad([it[n]["ids"] for n in ids]), "ilens": np.asarray([len(it[n]["ids"]) for n in ids], dtype=np.int64),
           "ys": pad([normalised(corpus, n, "mel") for n in ids]), "olens": np.asarray([it[n]["raw"]["mel"].shape[0] for n in ids], dtype=np.int64),
           "spkembs": None}
    for name, key in (("pitch", "pitch"), ("energy", "energys")):
        if name in feat_list:
            out[key] = pad([normalised(corpus, n, name) for n in ids])
            out[name + "_lens"] = out["ilens"].copy()
    if durations:
        out["durations"] = pad([it[n]["dur"] for n in ids])
        out["durations_lens"] = out["ilens"].copy()
        out["duration_lens"] = out["ilens"].copy()
    if "spkemb" in feat_list:
        out["spkembs"] = np.stack([normalised(corpus, n, "spkemb")[0] for n in ids])
    return out
