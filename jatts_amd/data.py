"""Stage-3 data path: the training set resident in HBM, a batch = one gather launch.

``ResidentDataset`` has the semantics of the reference's ``TTSDataset(is_inference=False)`` (jatts/datasets/tts_dataset.py:26-145) and
``BatchLoader`` those of ``DataLoader(dataset, batch_size, shuffle, collate_fn=FastSpeech2Collater())`` (jatts/bin/tts_train.py:231-273,
jatts/collaters/fastspeech2.py:17-107).  The reference reads one dump per utterance per step, normalises and pads on the CPU and copies to
the GPU; here every dump is read ONCE, every feature is one flat float32 store on the device, normalised once by the pinned
``features.standardize``, and a batch is ids -> ``hip.collate``: no feature byte crosses PCIe after loading.
"""
import csv
import logging

import numpy as np
import torch

from . import features, hip
from .bin.compute_statistics import read_feature, shaped
from .bin.tts_decode import TokenIDConverter, read_stats

_ENCODEC = ("encodec", "encodec_24khz", "encodec_48khz")
_ROWS_OF_TOKENS = ("pitch", "energy")      # token-averaged (FastSpeech2 recipes): one row per token


def batch_geometry(index, ids):
    """Host part of a batch: ``index`` maps a store name to its numpy ``row_len``; -> (length vectors as int64 numpy arrays, t_max per store).
    Everything a batch needs besides the gather comes from here, so none of it touches the device."""
    ids = np.asarray(ids, dtype=np.int64)
    lens = {k: v[ids].astype(np.int64) for k, v in index.items()}
    return lens, {k: int(v.max()) for k, v in lens.items()}


class ResidentDataset:
    """csv (``feat_path``, the token column, ``durations`` when present) + stats + token list -> device stores.

    ``stores``: name -> ``hip.CollateSource``: ``tokens`` (int64, (rows, 1)), ``durations`` (int64, (rows, 1); only with the csv column) and
    every feature of ``feat_list`` as float32 (rows, dim), normalised; ``pitch`` / ``energy`` are (rows, 1), ``spkemb`` one row of ``dim`` per
    utterance, as the reference shapes them (tts_dataset.py:129-145).  A dump's values are cast to float32 before the transform (the recipes'
    dumps are float32; the reference would carry a float64 dump through in float64 and round afterwards)."""

    def __init__(self, csv_path, stats_path, feat_list, token_list_path, token_column, device="cuda", prompt_feat_list=None,
                 prompt_strategy="same", resident_gb=64.0):
        feat_list = list(feat_list)
        for name in feat_list + list(prompt_feat_list or []):
            if name in _ENCODEC:
                raise ValueError(f"feature {name!r}: the encodec* features (codec-token models) are not part of the resident data path")
        if prompt_feat_list:
            raise ValueError("prompt_feat_list: prompt features are not part of the resident data path")
        if prompt_strategy == "given":
            raise ValueError("prompt_strategy: given is not part of the resident data path (only 'same', without prompt features)")
        if "mel" not in feat_list:
            raise ValueError("feat_list needs 'mel': the collater's ys (collaters/fastspeech2.py:54)")
        self.feat_list, self.token_column, self.device = feat_list, token_column, torch.device(device)
        self.converter = TokenIDConverter(token_list_path)
        with open(csv_path, newline="") as f:
            self.items = list(csv.DictReader(f))
        if not self.items:
            raise ValueError(f"{csv_path}: no utterances")
        self.has_durations = "durations" in self.items[0]

        tokens, durations, feats = [], [], {k: [] for k in feat_list}
        for n, it in enumerate(self.items):
            sid = it.get("sample_id", it.get("id", str(n)))
            ids = self.converter.tokens2ids([p for p in it[token_column].split(" ") if p != ""])      # tts_dataset.py:108-116
            if not ids:
                raise ValueError(f"{sid}: an empty utterance (no tokens in column {token_column!r})")
            tokens.append(np.asarray(ids, dtype=np.int64))
            arrays = {}
            for name in feat_list:
                try:
                    arrays[name] = np.ascontiguousarray(shaped(name, read_feature(it["feat_path"], name)), dtype=np.float32)
                except KeyError:
                    raise ValueError(f"{sid}: feature {name!r} missing from {it['feat_path']}") from None
            n_frames = arrays["mel"].shape[0]
            if n_frames < 1:
                raise ValueError(f"{sid}: an empty utterance (no mel rows)")
            for name in _ROWS_OF_TOKENS:
                if name in arrays and arrays[name].shape[0] != len(ids):
                    raise ValueError(f"{sid}: {name} has {arrays[name].shape[0]} rows, the utterance {len(ids)} tokens")
            if self.has_durations:
                d = np.asarray([int(v) for v in it["durations"].split(" ")], dtype=np.int64)          # tts_dataset.py:119-122
                if len(d) != len(ids):
                    raise ValueError(f"{sid}: {len(d)} durations for {len(ids)} tokens")
                if int(d.sum()) != n_frames:
                    raise ValueError(f"{sid}: durations sum to {int(d.sum())}, mel has {n_frames} rows")
                durations.append(d)
            for name in feat_list:
                feats[name].append(arrays[name])
            it["tokens"] = ids

        stats = {name: read_stats(stats_path, name) for name in feat_list}                                # tts_dataset.py:69-78
        self._build(tokens, durations if self.has_durations else None, feats, stats, resident_gb)
        logging.info(f"{csv_path}: {len(self.items)} utterances, {self.nbytes / 2 ** 20:.1f} MiB resident on {self.device}")

    @classmethod
    def from_arrays(cls, tokens, feats, stats, durations=None, device="cuda", resident_gb=64.0):
        """The same resident stores from arrays already in memory (benchmarks, tests): ``tokens`` a list of int64 id arrays, ``feats`` name -> list
        of float32 (rows, dim) arrays shaped as the dataset shapes them, ``stats`` name -> {"mean", "scale"}, ``durations`` a list of int64 arrays."""
        self = cls.__new__(cls)
        self.feat_list, self.token_column, self.device = list(feats), None, torch.device(device)
        self.items = [{"sample_id": str(n)} for n in range(len(tokens))]
        self.has_durations = durations is not None
        self._build([np.asarray(t, dtype=np.int64) for t in tokens], durations, feats, stats, resident_gb)
        return self

    def _build(self, tokens, durations, feats, stats, resident_gb):
        total = sum(a.nbytes for a in tokens) + sum(a.nbytes for a in durations or []) + sum(a.nbytes for v in feats.values() for a in v)
        if total > float(resident_gb) * 2 ** 30:
            raise ValueError(f"the training set takes {total / 2 ** 30:.2f} GiB on the device, above resident_gb = {resident_gb}")
        self.nbytes = total
        self.stores, self.stats = {}, {}
        self.stores["tokens"] = self._store(tokens, torch.int64)
        if durations is not None:
            self.stores["durations"] = self._store(durations, torch.int64)
        for name in self.feat_list:
            st = self.stats[name] = stats[name]
            dim = feats[name][0].shape[1]
            if any(a.shape[1] != dim for a in feats[name]) or st["mean"].size != dim or st["scale"].size != dim:
                raise ValueError(f"feature {name!r}: the dumps and the statistics disagree on the dimension ({dim} / {st['mean'].size})")
            self.stores[name] = self._store(feats[name], torch.float32, st)
        self.index = {k: s.row_len_host for k, s in self.stores.items()}

    def _store(self, arrays, dtype, stats=None):
        lens = np.asarray([a.shape[0] for a in arrays], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(lens)[:-1]])
        flat = np.concatenate([a.reshape(a.shape[0], -1) for a in arrays], axis=0)
        x = torch.from_numpy(flat).to(self.device)
        if stats is not None:
            x = features.standardize(x, stats["mean"], stats["scale"])                                  # StandardScaler.transform, once
        assert x.dtype == dtype
        return hip.CollateSource(x.contiguous(), start, lens)

    def __len__(self):
        return len(self.items)


class BatchLoader:
    """Batches of ``dataset`` as ``FastSpeech2Collater`` returns them, composed by torch's own samplers (``drop_last=False``, as the
    reference's ``DataLoader``): ``RandomSampler`` (``shuffle``; with ``seed`` a generator of its own, else torch's global one, as
    ``DataLoader(shuffle=True)`` draws) or ``SequentialSampler``; ``DistributedSampler`` when ``world_size > 1`` (tts_train.py:238-253).

    Per batch: ids -> length vectors and t_max from the host index -> ids staged through ``hip.h2d`` -> ONE ``jatts_collate`` launch into
    ``torch.empty`` outputs.  xs / ys / pitch / energys / durations / spkembs are device tensors, the ``*lens`` CPU int64 tensors (what the
    trainers' ``_signature`` reads).  The reference's collater writes ``durations_lens`` and its trainers read ``duration_lens``: both are here."""

    def __init__(self, dataset, batch_size, shuffle, seed=None, rank=0, world_size=1):
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        self.dataset, self.batch_size = dataset, int(batch_size)
        if world_size > 1:
            from torch.utils.data.distributed import DistributedSampler
            self.sampler = DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=bool(shuffle), seed=0 if seed is None else int(seed))
        elif shuffle:
            g = None if seed is None else torch.Generator().manual_seed(int(seed))
            self.sampler = RandomSampler(dataset, generator=g)
        else:
            self.sampler = SequentialSampler(dataset)
        self.batch_sampler = BatchSampler(self.sampler, self.batch_size, False)
        names = ["tokens", "mel"] + [k for k in ("pitch", "energy", "durations", "spkemb") if k in dataset.stores]
        self._names = names
        self._sources = [dataset.stores[k] for k in names]
        self._index = {k: dataset.index[k] for k in names}

    def set_epoch(self, epoch):
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for ids in self.batch_sampler:
            yield self.collate(ids)

    def collate(self, ids):
        lens, t_max = batch_geometry(self._index, ids)
        dev = self.dataset.device
        utt = hip.h2d([int(i) for i in ids], torch.int32, dev)
        outs = dict(zip(self._names, hip.collate(self._sources, ids, [t_max[k] for k in self._names], utt=utt)))
        B = len(ids)
        as_lens = lambda k: torch.from_numpy(lens[k])
        items = {"xs": outs["tokens"].view(B, -1), "ilens": as_lens("tokens"), "ys": outs["mel"], "olens": as_lens("mel"), "spkembs": None}
        if "pitch" in outs:
            items["pitch"], items["pitch_lens"] = outs["pitch"], as_lens("pitch")
        if "energy" in outs:
            items["energys"], items["energy_lens"] = outs["energy"], as_lens("energy")
        if "durations" in outs:
            items["durations"] = outs["durations"].view(B, -1)
            items["durations_lens"] = as_lens("durations")
            items["duration_lens"] = items["durations_lens"]
        if "spkemb" in outs:
            items["spkembs"] = outs["spkemb"].view(B, -1)
        return items
