#!/usr/bin/env python3
"""Stage-3 training CLI -- drop-in for ``jatts/bin/tts_train.py`` (reference :44-408) on the MI355X path.

Same flags (``--train-csv --dev-csv --stats --token-list --token-column --outdir --config [--pretrain] [--resume] [--verbose]``, rank and
world size from ``RANK`` / ``WORLD_SIZE``), same outputs (``<outdir>/config.yml`` with ``idim`` injected, ``checkpoint-<steps>steps.pkl`` in
the reference's format, ``predictions/<steps>steps/``).  Additive: ``--precision`` / ``--attention-precision`` (the trainers' arithmetic),
``--seed`` (default: unseeded, as the reference) and ``--resident-gb`` (the budget of the resident training set).

The training set lives on the device (``jatts_amd.data.ResidentDataset``); a batch is one gather launch (``BatchLoader``); the loop is
``jatts_amd.training.run_training``.  Options the trainers cannot honour are refused by name at start-up (``training.trainer_kwargs``);
``pin_memory``, ``num_workers`` and ``allow_cache`` are accepted and have no effect.  ``capture_graph`` stays off: random batches never
repeat a signature.

    python -m jatts_amd.bin.tts_train --config conf/fastspeech2.v1.yaml --train-csv data/train_raw_feat.csv --dev-csv data/dev_raw_feat.csv \\
        --stats exp/stats.npz --token-list exp/tokens.txt --token-column phonemes --outdir exp
"""
import argparse
import logging
import os
import sys

import torch
import yaml

import jatts_amd.models
from jatts_amd import training
from jatts_amd.bin.tts_decode import read_stats
from jatts_amd.data import BatchLoader, ResidentDataset


def get_parser():
    p = argparse.ArgumentParser(description="Train TTS model (MI355X HIP path).")
    p.add_argument("--train-csv", required=True, type=str, help="training csv file.")
    p.add_argument("--dev-csv", required=True, type=str, help="development csv file.")
    p.add_argument("--stats", required=True, type=str, help="stats file for normalization / denormalization (.npz, or .h5 with h5py).")
    p.add_argument("--token-list", required=True, type=str, help="a text mapping int-id to token")
    p.add_argument("--token-column", required=True, type=str, help="which column to use as the text input in the csv file")
    p.add_argument("--outdir", required=True, type=str, help="directory to save checkpoints.")
    p.add_argument("--config", required=True, type=str, help="yaml format configuration file.")
    p.add_argument("--pretrain", default="", type=str, nargs="?", help="checkpoint file path to load pretrained params.")
    p.add_argument("--resume", default="", type=str, nargs="?", help="checkpoint file path to resume training.")
    p.add_argument("--verbose", type=int, default=1, help="logging level. higher is more logging.")
    p.add_argument("--precision", default="fp32", choices=list(training.TRAIN_PRECISIONS), help="the trainers' arithmetic (extension)")
    p.add_argument("--attention-precision", default=None, choices=list(training.TRAIN_ATTENTIONS),
                   help="arithmetic of the attention products, a switch of its own (extension)")
    p.add_argument("--seed", type=int, default=None, help="seed of torch's generators and of the shuffle (extension; default: unseeded)")
    p.add_argument("--resident-gb", type=float, default=64.0, help="largest training set, in GiB, kept resident on the device (extension)")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    args.pretrain, args.resume = args.pretrain or "", args.resume or ""
    world = int(os.environ.get("WORLD_SIZE", 1))
    rank = int(os.environ.get("RANK", 0))
    distributed = world > 1
    level = logging.DEBUG if args.verbose > 1 else logging.INFO if args.verbose > 0 else logging.WARN
    if rank != 0:
        level = logging.WARN                        # the reference silences the other ranks' stdout (tts_train.py:133-135)
    logging.basicConfig(level=level, stream=sys.stdout, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    logging.info(f"World size: {world}")
    logging.info(f"Local rank: {rank}")
    if not torch.cuda.is_available():
        raise RuntimeError("jatts_amd needs an MI355X: there is no CPU fallback")
    shared = os.environ.get("JATTS_SHARED_GPU") == "1"          # tests only: every rank on cuda:0
    device = torch.device("cuda", 0 if shared else int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    if distributed:
        # (ranks that share one device -- the tests' world 2 on a one-GPU box -- exchange over gloo: RCCL refuses two ranks on one device)
        torch.distributed.init_process_group(backend="gloo" if shared else "nccl", init_method="env://")
        rank = torch.distributed.get_rank()
    if args.seed is not None:
        torch.manual_seed(args.seed)

    os.makedirs(args.outdir, exist_ok=True)
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    config.update(vars(args))
    config.update(rank=rank, world_size=world, distributed=distributed)
    with open(args.token_list, encoding="utf-8") as f:
        vocab_size = len([line.rstrip() for line in f])
    logging.info(f"Vocabulary size: {vocab_size}")
    config["model_params"]["idim"] = vocab_size                 # tts_train.py:185-190

    # everything the trainers cannot do is refused here, before anything is loaded or written
    trainer_class, kw = training.trainer_kwargs(config)
    if config.get("collater_type", "FastSpeech2Collater") != "FastSpeech2Collater":
        raise ValueError(f"collater_type: {config['collater_type']!r} is not implemented (FastSpeech2Collater)")
    if not hasattr(jatts_amd.models, config.get("model_type", "TransformerTTS")):
        raise ValueError(f"model_type: {config.get('model_type', 'TransformerTTS')!r} is not on the HIP path")
    for k in training.unread_keys(config, cli_keys=list(vars(args)) + ["rank", "world_size", "distributed"]):
        logging.warning(f"{k} = {config[k]} is not read by tts_train.")
    for k in training.NO_EFFECT_KEYS:
        if k in config:
            logging.info(f"{k} = {config[k]} has no effect: the training set is resident on the device.")

    if rank == 0:
        with open(os.path.join(args.outdir, "config.yml"), "w") as f:
            yaml.dump(config, f, Dumper=yaml.Dumper)
    for key, value in config.items():
        logging.info(f"{key} = {value}")

    ds_kw = dict(stats_path=args.stats, feat_list=config["feat_list"], token_list_path=args.token_list, token_column=args.token_column,
                 device=device, prompt_feat_list=config.get("prompt_feat_list"), prompt_strategy=config.get("prompt_strategy", "same"),
                 resident_gb=args.resident_gb)
    train_set = ResidentDataset(args.train_csv, **ds_kw)
    logging.info(f"The number of training files = {len(train_set)}.")
    training.check_durations(config, train_set.has_durations)
    dev_set = ResidentDataset(args.dev_csv, **ds_kw)
    logging.info(f"The number of development files = {len(dev_set)}.")
    train_loader = BatchLoader(train_set, config["batch_size"], shuffle=True, seed=args.seed, rank=rank, world_size=world)
    dev_loader = BatchLoader(dev_set, config["batch_size"], shuffle=False, rank=rank, world_size=world)

    model = getattr(jatts_amd.models, config["model_type"])(**config["model_params"])
    training.initialize_parameters(model, config["model_params"].get("init_type", "xavier_uniform"))      # the classes are built all-zero
    model = model.to(device)
    vocoder = None
    vcfg = config.get("vocoder") or None
    if vcfg and all(os.path.exists(str(vcfg.get(k, ""))) for k in ("checkpoint", "config", "stats")):
        from jatts_amd.vocoder import Vocoder
        vocoder = Vocoder(vcfg["checkpoint"], vcfg["config"], vcfg["stats"], device, trg_stats=read_stats(args.stats, config["out_feat_type"]))
    elif vcfg:
        logging.info("The vocoder's files do not exist: intermediate waveforms are skipped.")
    else:
        vocoder = training.griffin_lim_fallback(config, lambda: read_stats(args.stats, config["out_feat_type"]), device)

    trainer = trainer_class(model, precision=args.precision, attention=args.attention_precision, capture_graph=False, **kw)
    logging.info(model)
    epochs = 0
    if args.pretrain:
        trainer.load_checkpoint(args.pretrain, load_only_params=True)
        logging.info(f"Successfully load parameters from {args.pretrain}.")
    if args.resume:
        epochs = int(torch.load(args.resume, map_location="cpu").get("epochs", 0))
        trainer.load_checkpoint(args.resume)
        logging.info(f"Successfully resumed from {args.resume}.")
    # one model on every rank: the initial draws above are per rank (and --pretrain / --resume may name rank-local files); the reference gets this from
    # DistributedDataParallel's construction-time broadcast (tts_train.py:355-363).  After the trainer exists: its flat views receive the values.
    training.broadcast_model(model)
    training.run_training(trainer, train_loader, dev_loader, config, args.outdir, rank=rank, vocoder=vocoder, epochs=epochs)
    if distributed:
        spread = training.replica_spread(trainer)
        logging.info(f"Replica spread of the parameter sum over {world} ranks at exit: {spread:.3e}.")
        if spread != 0.0:
            logging.warning("The ranks' models differ: the checkpoints hold rank 0's.")
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
