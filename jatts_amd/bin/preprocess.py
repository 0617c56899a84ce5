"""Stage 1, first half: read the audio, resample it, extract and dump the raw features (the reference's ``jatts/bin/preprocess.py``)
on the GPU.

Same flags (``--csv --dumpdir --config [--f0_path] [--verbose]``, preprocess.py:39-66) plus ``--batch-size`` (utterances per ragged
launch, default 32) and ``--dump-format`` (``npz``, the default and the pinned path, or ``h5`` where h5py is importable: unpinned).
The config keys are the recipes': ``sampling_rate``, ``fft_size``, ``hop_size``, ``win_length``, ``window``, ``num_mels``, ``fmin``,
``fmax``, ``global_gain_scale``, ``feat_list``, ``log_base``; for pitch ``pitch_extract_type``, ``pitch_extract_f0min``,
``pitch_extract_f0max`` and, optionally, ``pitch_voicing_threshold``, ``pitch_silence_threshold``, ``pitch_octave_cost``.

Per batch the utterances are grouped by their files' native rate and every group is read -> ``jatts_resample`` ->
``jatts_wave_gain_peak`` -> ``LogMelExtractor`` in batched, ragged launches (``features.read_audio_batch``).  ``energy`` runs through
``features.Energy`` (the csv must carry ``durations``), ``spkemb`` through ``spkemb.SpkEmbExtractor`` with its "unverified" warning.
``pitch`` runs through ``features.Pitch`` when ``pitch_extract_type`` is ``acf``: this package's own autocorrelation estimator, whose parity
with the reference's DIO + StoneMask is UNPINNED (a warning says so); the steps after the raw track are the reference's.  The f0 range
comes from ``--f0_path`` by speaker (``item["spk"]``) or from the config (preprocess.py:263-270), a batch's utterances are grouped by their
range, and the csv must carry ``durations``.  ``pitch_extract_type: dio`` (pyworld) and the ``encodec*`` types (the encodec package) are
refused with a NotImplementedError before any file is written; a ``--f0_path`` without ``pitch`` in the list is accepted and ignored.

Every kept utterance becomes ``<dumpdir>/<sample_id>.npz`` (entries ``wave``, ``mel``, ... in float32: what
``jatts_amd.bin.compute_statistics`` reads), written once, and the csv is rewritten with a ``feat_path`` column
(preprocess.py:324-327).  An utterance whose gain clips is skipped with the reference's warning.

The sample-rate conversion is pinned on scipy.signal.resample_poly; parity with the reference's librosa.load(sr=...) (soxr_hq) is
UNPINNED, and so are the .h5 dumps.

    python -m jatts_amd.bin.preprocess --csv data/train.csv --dumpdir dump/train/feats --config conf/matcha_tts.mas.v1.yaml
"""
import argparse
import csv
import logging
import os

import numpy as np
import torch
import yaml

from jatts_amd import features

_LOG_FORMAT = "%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s"
_MISSING = {
    "pitch": "feat_list holds 'pitch': the reference extracts it with DIO through pyworld, which is not installed here and has no "
             "kernel in this package; remove 'pitch' from feat_list or run the reference's preprocess.py for this config. "
             "pitch_extract_type: acf selects this package's own autocorrelation estimator (parity with DIO unpinned).",
    "encodec": "feat_list holds '{}': EnCodec tokens need the encodec package, which is not installed here and has no kernel in this package",
}
_ENCODEC = ("encodec", "encodec_24khz", "encodec_48khz")
_ACF_WARNING = ("pitch_extract_type acf: F0 comes from this package's own autocorrelation estimator; parity with the reference's DIO + "
                "StoneMask is UNPINNED (the steps after the raw track are pinned on the reference)")


def check_feat_list(config):
    """The feature types this CLI serves, in the config's order.  Raises before anything is written: NotImplementedError for DIO pitch and
    encodec*, ValueError for the extractor types the reference refuses too (preprocess.py:122-150).  pitch_extract_type acf is accepted
    with a warning that its parity with DIO is unpinned."""
    feats = list(config.get("feat_list", ["mel"]))
    warned = False
    for f in feats + list(config.get("prompt_feat_list", [])):
        if f == "pitch":
            kind = config.get("pitch_extract_type")
            if kind in (None, "dio"):
                raise NotImplementedError(_MISSING["pitch"])
            if kind != "acf":
                raise ValueError(f"Unsupported pitch extractor type: {kind}")       # preprocess.py:123-125
            if not warned:
                logging.warning(_ACF_WARNING)
                warned = True
        if f in _ENCODEC:
            raise NotImplementedError(_MISSING["encodec"].format(f))
    if "energy" in feats and config.get("energy_extract_type") != "energy":
        raise ValueError(f"Unsupported energy extractor type: {config.get('energy_extract_type')}")
    if "spkemb" in feats and config.get("spkemb_extract_type") != "speechbrain":
        raise ValueError(f"Unsupported speaker embedding extractor type: {config.get('spkemb_extract_type')}")
    if "spkemb" in feats and not spkemb_checkpoint(config):       # (the reference downloads it; as in jatts_amd.bin.tts_decode)
        raise RuntimeError("feat_list has 'spkemb': set spkemb_checkpoint (config) or JATTS_SPKEMB_CHECKPOINT to SpeechBrain's ECAPA "
                           "embedding_model.ckpt")
    return feats


def spkemb_checkpoint(config):
    return config.get("spkemb_checkpoint") or os.environ.get("JATTS_SPKEMB_CHECKPOINT")


def _h5_writer():
    try:
        import h5py
    except ImportError as e:
        raise ImportError("--dump-format h5 needs h5py; dump .npz (the default)") from e

    def write(path, entries):
        with h5py.File(path, "w") as f:
            for k, v in entries.items():
                f.create_dataset(k, data=v)
    return write


def _write_npz(path, entries):
    with open(path, "wb") as f:
        np.savez(f, **entries)


def _none_if_empty(v):
    return None if v is None or str(v).strip() == "" else v


def main(argv=None):
    p = argparse.ArgumentParser(description="Preprocess audio and then extract features on the GPU (see jatts_amd/bin/preprocess.py).")
    p.add_argument("--csv", required=True, type=str, help="csv file.")
    p.add_argument("--dumpdir", type=str, required=True, help="directory to dump feature files.")
    p.add_argument("--config", type=str, required=True, help="yaml format configuration file.")
    p.add_argument("--f0_path", default=None, type=str, help="file storing f0 ranges (read only when feat_list holds pitch)")
    p.add_argument("--verbose", type=int, default=1, help="logging level. higher is more logging. (default=1)")
    p.add_argument("--batch-size", type=int, default=32, help="utterances per ragged launch (default=32)")
    p.add_argument("--dump-format", choices=("npz", "h5"), default="npz", help="npz (default, pinned) or h5 (needs h5py; unpinned)")
    args = p.parse_args(argv)
    if args.verbose > 1:
        logging.basicConfig(level=logging.DEBUG, format=_LOG_FORMAT)
    elif args.verbose > 0:
        logging.basicConfig(level=logging.INFO, format=_LOG_FORMAT)
    else:
        logging.basicConfig(level=logging.WARN, format=_LOG_FORMAT)
        logging.warning("Skip DEBUG/INFO messages")
    if args.batch_size < 1:
        raise ValueError("--batch-size must be positive")

    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    with open(args.csv, newline="") as f:
        dataset = list(csv.DictReader(f))

    # everything that can refuse does so here, before the first file is written
    feats = check_feat_list(config)
    known = [f for f in feats if f in ("mel", "pitch", "energy", "spkemb")]
    for f in feats:
        if f not in known:
            logging.info(f"Not supported feature type {f}. Skip.")
    for f, averaged in (("energy", "energy"), ("pitch", "f0")):
        if f in known and any(_none_if_empty(item.get("durations")) is None for item in dataset):
            raise ValueError(f"feat_list holds '{f}': every row of the csv needs a durations column (token-averaged {averaged})")
    f0_all = None
    if "pitch" in known and args.f0_path is not None:                      # preprocess.py:94-99
        with open(args.f0_path) as f:
            f0_all = yaml.load(f, Loader=yaml.Loader)
        for item in dataset:
            if item.get("spk") not in f0_all:
                raise KeyError(f"{args.f0_path} has no f0 range for speaker {item.get('spk')!r} ({item.get('sample_id')})")
    write = _h5_writer() if args.dump_format == "h5" else _write_npz
    if not dataset:
        raise ValueError(f"{args.csv} lists no utterance")

    device = torch.device("cuda")
    sr = config["sampling_rate"]
    stft = features.Stft(device, config["fft_size"], config["hop_size"], config["win_length"], config["window"]) \
        if "mel" in known or "energy" in known else None                      # one front end (one DFT table) serves both
    ex_mel = features.LogMelExtractor(device, sr, num_mels=config["num_mels"], fmin=config["fmin"], fmax=config["fmax"],
                                      log_base=config.get("log_base", 10.0), stft=stft) if "mel" in known else None
    ex_energy = features.Energy(fs=sr, n_fft=config["fft_size"], win_length=config["win_length"], hop_length=config["hop_size"],
                                window=config["window"], use_token_averaged_energy=True,
                                reduction_factor=config["model_params"]["reduction_factor"], stft=stft) if "energy" in known else None
    ex_pitch = None
    if "pitch" in known:
        ex_pitch = features.Pitch(fs=sr, n_fft=config["fft_size"], hop_length=config["hop_size"], use_token_averaged_f0=True,
                                  use_continuous_f0=True, use_log_f0=True, reduction_factor=config["model_params"]["reduction_factor"],
                                  voicing_threshold=config.get("pitch_voicing_threshold", features.PITCH_VOICING_THRESHOLD),
                                  silence_threshold=config.get("pitch_silence_threshold", features.PITCH_SILENCE_THRESHOLD),
                                  octave_cost=config.get("pitch_octave_cost", features.PITCH_OCTAVE_COST), device=device)

        def f0_range(item):                                                  # preprocess.py:263-270
            if f0_all is not None:
                return f0_all[item["spk"]]["f0min"], f0_all[item["spk"]]["f0max"]
            return config["pitch_extract_f0min"], config["pitch_extract_f0max"]
        for rng in sorted({f0_range(item) for item in dataset}):             # a range the geometry refuses ends the run here
            features.pitch_geometry(sr, config["fft_size"], *rng)
    ex_spk = None
    if "spkemb" in known:
        from jatts_amd.spkemb import SpkEmbExtractor
        ex_spk = SpkEmbExtractor(device, checkpoint=spkemb_checkpoint(config), **config.get("spkemb_params", {}))       # ECAPA_TDNN kwargs

    os.makedirs(args.dumpdir, exist_ok=True)
    new_datas = []
    for b0 in range(0, len(dataset), args.batch_size):
        batch = dataset[b0:b0 + args.batch_size]
        waves = features.read_audio_batch(
            [(item["wav_path"], _none_if_empty(item.get("start")), _none_if_empty(item.get("end"))) for item in batch],
            sr, config["global_gain_scale"], device)
        kept = []
        for item, w in zip(batch, waves):
            if w is None:
                logging.warning(f"{item['wav_path']} returns None. Skip.")
            else:
                kept.append((item, w))
        if not kept:
            continue
        durations = None
        if _none_if_empty(kept[0][0].get("durations")) is not None:
            durations = [None if _none_if_empty(item.get("durations")) is None else [int(d) for d in item["durations"].split(" ")]
                         for item, _ in kept]
        pw = features.PackedWaves.from_list([w for _, w in kept], device)
        entries = [{"wave": w.cpu().numpy().astype(np.float32)} for _, w in kept]
        if ex_mel is not None:
            rb, mel = ex_mel(pw)
            mel = mel[:, :ex_mel.num_mels].cpu().numpy()
            for i, (item, _) in enumerate(kept):
                feat = mel[rb.cu_host[i]:rb.cu_host[i + 1]]
                if durations is not None and durations[i] is not None:      # check duration (preprocess.py:258-261)
                    total = sum(durations[i])
                    assert total == feat.shape[0], \
                        f"{item['sample_id']}: mel duration {feat.shape[0]} and phoneme durations {total} don't match ."
                entries[i]["mel"] = np.ascontiguousarray(feat, dtype=np.float32)
        if ex_pitch is not None:
            by_range = {}
            for i, (item, _) in enumerate(kept):
                by_range.setdefault(f0_range(item), []).append(i)
            for (f0min, f0max), members in by_range.items():                 # one ragged run per range, as read_audio_batch groups by rate
                sub = pw if len(members) == len(kept) else pw.select(members)
                # (feat_length = len(mel), preprocess.py:272-276: the track has the mel's frames already)
                pit = ex_pitch.extract(sub, f0min, f0max, None, [durations[i] for i in members])
                for i, v in zip(members, pit):
                    entries[i]["pitch"] = v.cpu().numpy().astype(np.float32)
        if ex_energy is not None:
            en = ex_energy.extract(pw, [sum(d) for d in durations], durations)
            for i, e in enumerate(en):
                entries[i]["energy"] = e.cpu().numpy().astype(np.float32)
        if ex_spk is not None:
            emb = ex_spk.forward_many([item["wav_path"] for item, _ in kept])
            for i in range(len(kept)):
                entries[i]["spkemb"] = np.asarray(emb[i], dtype=np.float32).reshape(-1)
        for (item, _), ent in zip(kept, entries):
            feat_path = os.path.join(args.dumpdir, f"{item['sample_id']}.{args.dump_format}")
            write(feat_path, ent)
            new_datas.append({**item, "feat_path": os.path.realpath(feat_path)})
        logging.info("%d / %d utterances done", min(b0 + args.batch_size, len(dataset)), len(dataset))

    if not new_datas:
        raise ValueError(f"no utterance of {args.csv} was kept")
    with open(args.csv, "w", newline="") as f:                               # write_csv (utils.py:87-100)
        writer = csv.DictWriter(f, fieldnames=list(new_datas[0].keys()))
        writer.writeheader()
        for line in new_datas:
            writer.writerow(line)


if __name__ == "__main__":
    main()
