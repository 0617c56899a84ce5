#!/usr/bin/env python3
"""collate_kat.npz: one batch of the REAL ``FastSpeech2Collater`` (jatts/collaters/fastspeech2.py, loaded by path: it imports numpy and torch
only) over three utterances normalised by the REAL sklearn ``StandardScaler.transform`` as ``TTSDataset.__getitem__`` applies it
(jatts/datasets/tts_dataset.py:124-145, on float32 dumps with the float32 statistics the stats file stores).

    python tests/golden/make_golden_collate.py /path/to/jatts-checkout

(tokens, frames) = (3, 7), (1, 1), (5, 12); mel dim 5, spkemb dim 4.  Stored: the raw dumps (``raw_<feat>_<n>``), token ids and durations per
utterance, the statistics, and every tensor of the collater's dict as ``batch_<key>`` (``spkembs`` included; keys in ``batch_keys``).
"""
import importlib.util
import json
import os
import sys

import numpy as np
from sklearn.preprocessing import StandardScaler

ref = sys.argv[1]
spec = importlib.util.spec_from_file_location("ref_collater", os.path.join(ref, "jatts", "collaters", "fastspeech2.py"))
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

rng = np.random.default_rng(20)
GEOM = [(3, 7), (1, 1), (5, 12)]
ODIM, SDIM = 5, 4
stats = {}
for name, dim in (("mel", ODIM), ("pitch", 1), ("energy", 1), ("spkemb", SDIM)):
    stats[name] = (rng.normal(0.0, 2.0, dim).astype(np.float32), rng.uniform(0.5, 3.0, dim).astype(np.float32))

out, items = {}, []
for n, (nt, nf) in enumerate(GEOM):
    cuts = np.sort(rng.choice(np.arange(1, nf), nt - 1, replace=False)) if nt > 1 else np.array([], dtype=np.int64)
    dur = np.diff(np.concatenate([[0], cuts, [nf]])).astype(np.int64)
    assert dur.sum() == nf and len(dur) == nt and dur.min() >= 1
    raw = {"mel": rng.normal(0.0, 3.0, (nf, ODIM)).astype(np.float32), "pitch": rng.normal(5.0, 1.0, nt).astype(np.float32),
           "energy": rng.normal(0.0, 1.0, nt).astype(np.float32), "spkemb": rng.normal(0.0, 1.0, SDIM).astype(np.float32)}
    raw["mel"][0, 0] = -0.0
    item = {"token_indices": rng.integers(2, 9, nt).astype(np.int64), "durations_int": dur}
    for name, x in raw.items():
        out[f"raw_{name}_{n}"] = x
        x2 = x.reshape(1, -1) if name == "spkemb" else x.reshape(-1, 1) if name in ("pitch", "energy") else x      # tts_dataset.py:129-135
        sc = StandardScaler()
        sc.mean_, sc.scale_ = stats[name]
        y = sc.transform(x2)
        assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), ((x2 - stats[name][0]) / stats[name][1]).view(np.uint32))
        item[name] = np.squeeze(y, 0) if name == "spkemb" else y
    out[f"tokens_{n}"], out[f"durations_{n}"] = item["token_indices"], dur
    items.append(item)

batch = mod.FastSpeech2Collater()(items)
keys = []
for k, v in batch.items():
    out[f"batch_{k}"] = v.numpy()
    keys.append([k, str(v.dtype), list(v.shape)])
out["batch_keys"] = json.dumps(keys)
for name, (m, s) in stats.items():
    out[f"{name}_mean"], out[f"{name}_scale"] = m, s
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "collate_kat.npz")
np.savez(path, **out)
print(path, keys)
