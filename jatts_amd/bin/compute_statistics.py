"""Stage 1, second half: mean and scale of the dumped features (the reference's ``jatts/bin/compute_statistics.py``) on the GPU.

Same flags (``--csv --out [--verbose]``, compute_statistics.py:29-45).  Every row of the csv names a ``feat_path``; the feature
names are the entries of the first file (``wave`` is skipped), and every feature gets one ``features.FeatureStatistics``: one
``partial_fit`` per utterance, the running float64 state stays on the device, one read-back per feature at the end.  ``spkemb``
(dim,) counts as one row, ``pitch`` / ``energy`` (n_frames,) as one column (compute_statistics.py:85-91).

Dumps are read as ``.npz`` (always) or ``.h5`` (when h5py is importable); ``--out`` likewise: ``<feat>_mean`` / ``<feat>_scale``
float32, what ``jatts_amd.bin.tts_decode.read_stats`` and the later stages read.

    python -m jatts_amd.bin.compute_statistics --csv data/train.csv --out exp/stats.npz
"""
import argparse
import csv
import logging

import numpy as np
import torch

from jatts_amd import features

_LOG_FORMAT = "%(asctime)s %(levelname)s [%(module)s:%(lineno)d] %(message)s"


def _h5py():
    try:
        import h5py
    except ImportError as e:
        raise ImportError("reading .h5 features needs h5py; dump them as .npz (one entry per feature)") from e
    return h5py


def feature_names(path):
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return list(z.files)
    with _h5py().File(path, "r") as f:
        return list(f["/"].keys())


def read_feature(path, name):
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return z[name]
    with _h5py().File(path, "r") as f:
        return f[name][()]


def shaped(feat_name, feat):
    """compute_statistics.py:85-91: spkemb [dim] -> [1, dim]; pitch, energy [n_frames] -> [n_frames, 1]."""
    feat = np.asarray(feat)
    if feat_name == "spkemb":
        return feat.reshape(1, -1)
    if feat_name in ("pitch", "energy"):
        return feat.reshape(-1, 1)
    if feat.ndim != 2:
        raise ValueError(f"feature {feat_name!r} has shape {feat.shape}: (n_frames, dim) expected")
    return feat


def main(argv=None):
    p = argparse.ArgumentParser(description="Per-feature mean and scale of a list of feature dumps, accumulated on the GPU.")
    p.add_argument("--csv", required=True, help="csv with a feat_path column, one utterance per row")
    p.add_argument("--out", type=str, required=True, help="statistics file to write or update (.npz, or .h5 with h5py)")
    p.add_argument("--verbose", type=int, default=1, help="0: warnings only, 1: info, 2 and above: debug")
    args = p.parse_args(argv)
    if args.verbose > 1:
        logging.basicConfig(level=logging.DEBUG, format=_LOG_FORMAT)
    elif args.verbose > 0:
        logging.basicConfig(level=logging.INFO, format=_LOG_FORMAT)
    else:
        logging.basicConfig(level=logging.WARNING, format=_LOG_FORMAT)

    with open(args.csv, newline="") as f:
        dataset = list(csv.DictReader(f))
    if not dataset:
        raise ValueError(f"{args.csv} lists no utterance")
    logging.info("%d utterances listed", len(dataset))
    device = torch.device("cuda")
    for feat_name in feature_names(dataset[0]["feat_path"]):
        if feat_name == "wave":
            continue
        logging.info("accumulating %s", feat_name)
        acc = None
        for line in dataset:
            feat = shaped(feat_name, read_feature(line["feat_path"], feat_name))
            if acc is None:
                acc = features.FeatureStatistics(feat.shape[1], device)
            x = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).pin_memory().to(device, non_blocking=True)
            acc.partial_fit(x)
        acc.save(args.out, feat_name)


if __name__ == "__main__":
    main()
