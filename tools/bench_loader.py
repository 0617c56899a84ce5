#!/usr/bin/env python3
"""Measure the stage-3 data path at recipe size: a seeded synthetic resident set of 2 000 utterances with JSUT-like lengths,
odim 80, batch 32, FastSpeech2 at the FS2_JSUT width.

  (a) the loader alone: host time and device time per batch, achieved bytes/s of the gather against the HBM peak;
  (b) a STAND-IN for the host path, written here: the same (normalised) arrays in pinned host memory, padded with numpy in the main process and
      copied with ``.to(device, non_blocking=True)``.  It is not the reference's multi-worker DataLoader (no HDF5 read, no per-step
      StandardScaler, no worker processes): it is the cheapest form that path could take;
  (c) ``FastSpeech2Trainer.train_step`` on one fixed batch against loader-fed steps over the same number of steps, per trainer precision.

Variants alternate inside one call (``--rounds`` windows each); every window ends in a device synchronise inside the host clock; device time
comes from events.  The bytes are computed from the batch shapes: every output byte written once, every valid byte read once.

    python tools/bench_loader.py --out profiles/loader.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, spec; a float4 copy reaches 6.29e12


def synthetic_corpus(n_utt, odim, vocab, seed):
    rng = np.random.default_rng(seed)
    n_tok = np.clip(np.rint(rng.lognormal(np.log(55.0), 0.45, n_utt)), 8, 200).astype(np.int64)        # JSUT: ~5 s, ~55 phonemes an utterance
    tokens, durations, feats = [], [], {"mel": [], "pitch": [], "energy": []}
    for nt in n_tok:
        d = rng.integers(2, 13, int(nt)).astype(np.int64)                                               # ~7 frames a phoneme at 80 frames/s
        tokens.append(rng.integers(2, vocab - 1, int(nt)).astype(np.int64))
        durations.append(d)
        feats["mel"].append(rng.normal(0.0, 1.0, (int(d.sum()), odim)).astype(np.float32))
        feats["pitch"].append(rng.normal(0.0, 1.0, (int(nt), 1)).astype(np.float32))
        feats["energy"].append(rng.normal(0.0, 1.0, (int(nt), 1)).astype(np.float32))
    stats = {k: {"mean": np.zeros(v[0].shape[1], np.float32), "scale": np.ones(v[0].shape[1], np.float32)} for k, v in feats.items()}
    return tokens, durations, feats, stats


class HostStandIn:
    """(b): flat pinned host stores, numpy padding in the main process, non_blocking copies."""

    def __init__(self, tokens, durations, feats, device):
        self.device = device
        self.arr = {"xs": tokens, "durations": durations, "ys": feats["mel"], "pitch": feats["pitch"], "energys": feats["energy"]}
        self.pinned = {}
        for k, arrays in self.arr.items():                      # one pinned block per field; the utterances are views into it
            flat = torch.from_numpy(np.concatenate([a.reshape(a.shape[0], -1) for a in arrays])).pin_memory()
            views, o = [], 0
            fn = flat.numpy()
            for a in arrays:
                views.append(fn[o:o + a.shape[0]].reshape(a.shape))
                o += a.shape[0]
            self.pinned[k], self.arr[k] = flat, views

    def collate(self, ids):
        out = {}
        for k, arrays in self.arr.items():
            xs = [arrays[i] for i in ids]
            pad = np.zeros((len(xs), max(x.shape[0] for x in xs)) + xs[0].shape[1:], dtype=xs[0].dtype)
            for b, x in enumerate(xs):
                pad[b, :x.shape[0]] = x
            out[k] = torch.from_numpy(pad).to(self.device, non_blocking=True)
        out["ilens"] = torch.tensor([self.arr["xs"][i].shape[0] for i in ids])
        out["olens"] = torch.tensor([self.arr["ys"][i].shape[0] for i in ids])
        return out


def batch_bytes(batch, ds, ids):
    wr = sum(v.numel() * v.element_size() for v in batch.values() if torch.is_tensor(v) and v.is_cuda)
    rd = sum(int(s.row_len_host[ids].sum()) * s.src.shape[1] * s.src.element_size() for s in ds.stores.values())
    return wr + rd


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--utts", type=int, default=2000)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--odim", type=int, default=80)
    p.add_argument("--rounds", type=int, default=5, help="alternated windows per variant")
    p.add_argument("--loader-batches", type=int, default=252, help="batches per loader window (four epochs of 63)")
    p.add_argument("--steps", type=int, default=20, help="train steps per window")
    p.add_argument("--precisions", default="fp32,fp32_bf16x3")
    p.add_argument("--skip-train", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_loader measures on an MI355X: there is no CPU fallback")
    from jatts_amd import training
    from jatts_amd.data import BatchLoader, ResidentDataset
    from jatts_amd.models import FastSpeech2
    from jatts_amd.synthetic import FS2_JSUT

    dev, vocab = torch.device("cuda:0"), 45
    tokens, durations, feats, stats = synthetic_corpus(args.utts, args.odim, vocab, args.seed)
    ds = ResidentDataset.from_arrays(tokens, feats, stats, durations=durations, device=dev)
    loader = BatchLoader(ds, args.batch, shuffle=True, seed=args.seed)
    stand_in = HostStandIn(tokens, durations, feats, dev)
    id_lists = []
    while len(id_lists) < max(args.loader_batches, args.steps * args.rounds * 2 + 8):
        id_lists += [b for b in loader.batch_sampler if len(b) == args.batch]
    res = {"box": torch.cuda.get_device_name(0), "utts": args.utts, "batch": args.batch, "odim": args.odim,
           "resident_mib": ds.nbytes / 2 ** 20, "frames_mean": float(np.mean([m.shape[0] for m in feats["mel"]])),
           "frames_max": int(max(m.shape[0] for m in feats["mel"]))}

    # ---- (a) / (b): alternated windows over the same id lists
    window = id_lists[:args.loader_batches]
    for fn in (loader.collate, stand_in.collate):                # warm-up: code objects, allocator blocks, pinned staging
        for ids in window[:16]:
            fn(ids)
    torch.cuda.synchronize()
    a_host, a_wall, a_dev, a_rate, b_wall = [], [], [], [], []
    for _ in range(args.rounds):
        evs, nbytes = [], 0
        t0 = time.perf_counter()
        for ids in window:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            batch = loader.collate(ids)
            e1.record()
            evs.append((e0, e1))
            nbytes += batch_bytes(batch, ds, np.asarray(ids))
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dev_s = sum(e0.elapsed_time(e1) for e0, e1 in evs) * 1e-3
        a_host.append((t1 - t0) / len(window) * 1e6)
        a_wall.append((t2 - t0) / len(window) * 1e6)
        a_dev.append(dev_s / len(window) * 1e6)
        a_rate.append(nbytes / dev_s)
        t0 = time.perf_counter()
        for ids in window:
            stand_in.collate(ids)
        torch.cuda.synchronize()
        b_wall.append((time.perf_counter() - t0) / len(window) * 1e6)
    res["a_loader"] = {"host_us_per_batch": spread(a_host), "wall_us_per_batch": spread(a_wall),
                       "device_us_per_batch_events_around_h2d_and_gather": spread(a_dev), "bytes_per_s_over_event_time": spread(a_rate),
                       "share_of_hbm_peak": statistics.median(a_rate) / HBM_PEAK, "bytes_per_batch": nbytes / len(window)}
    res["b_host_stand_in"] = {"wall_us_per_batch": spread(b_wall), "note": "stand-in written in this tool, not the reference's multi-worker DataLoader"}
    print(json.dumps({"a_loader": res["a_loader"], "b_host_stand_in": res["b_host_stand_in"]}), flush=True)

    # ---- (c): fixed batch against loader-fed steps
    if not args.skip_train:
        res["c_train_step"] = {}
        for prec in [x for x in args.precisions.split(",") if x]:
            torch.manual_seed(args.seed)
            model = training.initialize_parameters(FastSpeech2(idim=vocab, **FS2_JSUT)).to(dev)
            tr = training.FastSpeech2Trainer(model, lr=1e-4, grad_norm=1.0, warmup_steps=4000, precision=prec)
            fixed = loader.collate(id_lists[0])
            feed = iter(id_lists[1:])
            for _ in range(3):                                   # warm-up both forms
                tr.train_step(fixed)
                tr.train_step(loader.collate(next(feed)))
            torch.cuda.synchronize()
            t_fixed, t_fed = [], []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.train_step(fixed)
                torch.cuda.synchronize()
                t_fixed.append((time.perf_counter() - t0) / args.steps * 1e3)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.train_step(loader.collate(next(feed)))
                torch.cuda.synchronize()
                t_fed.append((time.perf_counter() - t0) / args.steps * 1e3)
            res["c_train_step"][prec] = {"fixed_batch_ms": spread(t_fixed), "loader_fed_ms": spread(t_fed),
                                         "fixed_batch_frames": int(fixed["olens"].sum()), "fixed_batch_t_max": int(fixed["ys"].shape[1])}
            print(json.dumps({prec: res["c_train_step"][prec]}), flush=True)
            del tr, model
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
