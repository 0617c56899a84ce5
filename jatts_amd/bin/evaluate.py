"""Stage 5 of the recipes (objective evaluation) on the GPU: the reference's ``jatts/bin/evaluate.py`` for the metrics this package
computes.  Same flags (``--wavdir --csv --f0_path --metrics --n_jobs``; ``--n_jobs`` is accepted and unused: the pairs run as ragged
batches on one device), plus ``--batch-size``, ``--spkemb_checkpoint`` and ``--json PATH``.

  mcd     MCD, F0RMSE, F0CORR and DDUR per utterance (jatts_amd.evaluate: the definitions, and what is pinned on what)
  spkemb  cosine similarity of the ECAPA embeddings of ``wavdir/<id>.wav`` and the csv's ``ref_wav_path``; needs ``--spkemb_checkpoint``
  asr, sheet   refused by name at start-up: nue_asr and the SHEET hub model are not part of this package

Output, in this order: the definitions line, the reference's ``Mean ...`` line at INFO (the recipes grep "INFO: Mean"), a plain-text
per-utterance table sorted by sample id, and with ``--json`` the per-utterance values.

    python -m jatts_amd.bin.evaluate --wavdir exp/.../wav --csv data/test.csv --f0_path conf/f0.yaml --metrics mcd
"""
import argparse
import csv
import json
import logging
import os
import sys

import numpy as np

_LOG_FORMAT = "%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s"      # the reference's (evaluate.py:173-176)
_REFUSED = {
    "asr": "metric 'asr': CER needs the nue_asr model, which is not part of this package; run the reference's evaluate.py for it",
    "sheet": "metric 'sheet': the SHEET score needs the unilight/sheet hub model, which is not part of this package; run the reference's "
             "evaluate.py for it",
}
KNOWN_METRICS = ("mcd", "spkemb", "asr", "sheet")
MCD_COLUMNS = (("MCD", ".2f"), ("F0RMSE", ".3f"), ("F0CORR", ".3f"), ("DDUR", ".3f"))


def check_metrics(metrics, spkemb_checkpoint=None):
    """Refusals by name, before any file is read: asr and sheet (NotImplementedError), an unknown metric, spkemb without a checkpoint."""
    for m in metrics:
        if m in _REFUSED:
            raise NotImplementedError(_REFUSED[m])
        if m not in KNOWN_METRICS:
            raise ValueError(f"unknown metric {m!r} (this package computes: mcd, spkemb)")
    if "spkemb" in metrics and not spkemb_checkpoint:
        raise ValueError("metric 'spkemb' needs --spkemb_checkpoint: SpeechBrain's ECAPA embedding_model.ckpt (the reference downloads it)")
    return list(dict.fromkeys(metrics))


def get_parser():
    p = argparse.ArgumentParser(description="objective evaluation script (GPU; see jatts_amd/bin/evaluate.py).")
    p.add_argument("--wavdir", required=True, type=str, help="directory for converted waveforms")
    p.add_argument("--csv", type=str, required=True, help="path to csv file")
    p.add_argument("--f0_path", required=True, type=str, help="file storing f0 ranges")
    p.add_argument("--metrics", nargs="+", required=True, help="metrics to evaluate: mcd, spkemb")
    p.add_argument("--n_jobs", default=10, type=int, help="accepted for the reference's command lines; unused")
    p.add_argument("--batch-size", type=int, default=16, help="pairs per ragged batch (default=16)")
    p.add_argument("--spkemb_checkpoint", type=str, default=None, help="SpeechBrain ECAPA embedding_model.ckpt (metric spkemb)")
    p.add_argument("--json", type=str, default=None, help="write the per-utterance values to this file")
    return p


def format_table(ids, columns):
    """Aligned plain-text columns: ``columns`` = (title, format, {id: value}); rows sorted by sample id."""
    ids = sorted(ids)
    cells = [["Sample ID"] + [c[0] for c in columns]] + [[i] + [format(c[2][i], c[1]) for c in columns] for i in ids]
    width = [max(len(r[k]) for r in cells) for k in range(len(cells[0]))]
    return "\n".join("  ".join(v.ljust(width[0]) if k == 0 else v.rjust(width[k]) for k, v in enumerate(r)) for r in cells)


def run_mcd(dataset, wavdir, f0_all, batch_size, device="cuda"):
    """-> {sample id: {"MCD", "F0RMSE", "F0CORR", "DDUR"}}.  The generated file sets the rate; the ground truth is read through
    ``read_audio`` at that rate (evaluate.py:135-138).  Pairs are grouped by (rate, f0 range) and batched in order of length."""
    from jatts_amd import evaluate as ev
    from jatts_amd.features import read_audio_batch
    from jatts_amd.wavio import decode_wav

    groups = {}
    for item in dataset:
        sid, spk = item["sample_id"], item["spk"]
        a, fs = decode_wav(os.path.join(wavdir, sid + ".wav"))
        x = a[:, 0] if a.shape[1] == 1 else a.mean(axis=1, dtype=np.float32)
        key = (int(fs), float(f0_all[spk]["f0min"]), float(f0_all[spk]["f0max"]))
        start, end = (item.get("start") or None), (item.get("end") or None)
        groups.setdefault(key, []).append((sid, np.ascontiguousarray(x, dtype=np.float32), item["wav_path"],
                                           None if start is None else float(start), None if end is None else float(end)))
    e = ev.evaluator(device)
    results = {}
    for (fs, f0min, f0max), members in groups.items():
        members.sort(key=lambda m: m[1].size)
        for i in range(0, len(members), batch_size):
            chunk = members[i:i + batch_size]
            gts = read_audio_batch([(m[2], m[3], m[4]) for m in chunk], fs, device=device)
            if any(g is None for g in gts):
                raise ValueError("a ground-truth wave clips")      # (never: the gain is 1)
            res = e.evaluate_batch([(m[1], g, m[0]) for m, g in zip(chunk, gts)], fs, f0min, f0max)
            for m, r in zip(chunk, res):
                results[m[0]] = r
    return results


def run_spkemb(dataset, wavdir, checkpoint, device="cuda"):
    """-> {sample id: cosine of the embeddings of wavdir/<id>.wav and ref_wav_path} (hip.l2_normalize, hip.rowdot)"""
    import torch

    from jatts_amd import hip
    from jatts_amd._abi import F32
    from jatts_amd.spkemb import SpkEmbExtractor, load_wav

    ex = SpkEmbExtractor(device, checkpoint)
    ids = [item["sample_id"] for item in dataset]
    with torch.no_grad():
        gen = hip.l2_normalize(ex.encode_batch([load_wav(os.path.join(wavdir, i + ".wav"))[0] for i in ids]).contiguous(), F32)
        ref_paths = list(dict.fromkeys(item["ref_wav_path"] for item in dataset))
        ref = hip.l2_normalize(ex.encode_batch([load_wav(p)[0] for p in ref_paths]).contiguous(), F32)
        sims = {}
        for k, p in enumerate(ref_paths):      # one rowdot per reference file: every generated row against that file's unit vector
            rows = [n for n, item in enumerate(dataset) if item["ref_wav_path"] == p]
            sel = gen[rows].contiguous()
            dots = hip.rowdot(sel, sel.shape[1], len(rows), 1, sel.shape[1], ref[k:k + 1].contiguous()).reshape(-1).cpu().numpy()
            for n, v in zip(rows, dots):
                sims[ids[n]] = float(v)
    return sims


def main(argv=None):
    args = get_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format=_LOG_FORMAT)
    metrics = check_metrics(args.metrics, args.spkemb_checkpoint)      # before any file is read
    if args.batch_size < 1:
        raise ValueError("--batch-size must be positive")
    logging.info(f"--n_jobs {args.n_jobs} is accepted and unused: the pairs run as ragged batches on one device")

    import yaml

    from jatts_amd import evaluate as ev

    with open(args.csv, newline="") as f:
        dataset = list(csv.DictReader(f))
    logging.info("number of utterances = {}".format(len(dataset)))
    if "spkemb" in metrics and any("ref_wav_path" not in item for item in dataset):
        raise ValueError("metric 'spkemb' needs the csv's ref_wav_path column")
    with open(args.f0_path) as f:
        f0_all = yaml.load(f, Loader=yaml.FullLoader)

    ids = [item["sample_id"] for item in dataset]
    columns, per_utt = [], {i: {} for i in ids}
    means, sim_mean = None, None
    if "spkemb" in metrics:
        logging.info("Calculating speaker embedding cosine similarity...")
        sims = run_spkemb(dataset, args.wavdir, args.spkemb_checkpoint)
        sim_mean = float(np.mean(np.array([sims[i] for i in ids])))
        columns.append(("SPKEMB SIM", ".3f", sims))
        for i in ids:
            per_utt[i]["SPKEMB SIM"] = sims[i]
    if "mcd" in metrics:
        logging.info("Calculating MCD and f0-related scores...")
        res = run_mcd(dataset, args.wavdir, f0_all, args.batch_size)
        means = {k: float(np.mean(np.array([res[i][k] for i in ids]))) for k, _ in MCD_COLUMNS}      # a NaN propagates, as in the reference
        columns = [(k, fmt, {i: res[i][k] for i in ids}) for k, fmt in MCD_COLUMNS] + columns
        for i in ids:
            per_utt[i].update(res[i])
        logging.info(ev.DEFINITIONS)
    logging.info(ev.format_mean(means, sim_mean))
    print(format_table(ids, columns))
    sys.stdout.flush()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"mean": dict(means or {}, **({"SPKEMB SIM": sim_mean} if sim_mean is not None else {})), "utterances": per_utt}, f,
                      indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
