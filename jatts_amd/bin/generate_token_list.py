#!/usr/bin/env python3
"""Stage-2 token list -- ``jatts/bin/generate_token_list.py`` (reference :280-330) for the recipes' phoneme columns.

    python -m jatts_amd.bin.generate_token_list --csv data/train.csv --out dump/token_list/train_phn_julius/tokens.txt --column phonemes \\
        --non_linguistic_symbols none --cleaner none --add_symbol "<blank>:0" --add_symbol "<unk>:1" --add_symbol "<sos/eos>:-1"

The column is split at spaces; tokens are written by descending count, ties in the order of first appearance (a Counter keeps insertion
order and the sort is stable, as in the reference); ``--add_symbol "<tok>:<idx>"`` inserts at that index, ``-1`` appends.  Empty strings (two
spaces in a row) are not tokens: the dataset drops them too (``jatts_amd.data``).  Text cleaners, g2p and the character / word modes are not
here and are refused by name; ``--non_linguistic_symbols`` is accepted as the reference accepts it (its phoneme mode never reads it).
"""
import argparse
import csv
import logging
import os
from collections import Counter


def build_token_list(rows, add_symbol=(), cutoff=0):
    """rows: iterable of token strings (one utterance each) -> the token list."""
    counter = Counter()
    for text in rows:
        for t in text.split(" "):
            if t != "":
                counter[t] += 1
    words = [w for w, c in sorted(counter.items(), key=lambda x: -x[1]) if c > cutoff]
    for symbol_and_id in add_symbol:
        try:
            symbol, idx = symbol_and_id.rsplit(":", 1)
            idx = int(idx)
        except ValueError:
            raise RuntimeError(f"Format error: e.g. '<blank>:0': {symbol_and_id}") from None
        if idx < 0:
            idx = len(words) + 1 + idx
        words.insert(idx, symbol.strip())
    return words


def _none(v):
    return None if v is None or v.lower() in ("none", "null", "nil", "") else v


def get_parser():
    p = argparse.ArgumentParser(description="Token list of a csv column, most frequent first.")
    p.add_argument("--csv", required=True, help="csv file path")
    p.add_argument("--out", required=True, help="output token list path")
    p.add_argument("--column", required=True, help="which column of the input csv file to use")
    p.add_argument("--token_type", default="phn", help="Token type (phn)")
    p.add_argument("--non_linguistic_symbols", type=_none, default=None, help="non_linguistic_symbols file path (accepted, unused in phn mode)")
    p.add_argument("--cleaner", type=_none, default=None, help="text cleaner (only none)")
    p.add_argument("--g2p", type=_none, default=None, help="g2p (only none: the column holds phonemes already)")
    p.add_argument("--cutoff", default=0, type=int, help="cut-off frequency")
    p.add_argument("--add_symbol", type=str, default=[], action="append", help="e.g. --add_symbol '<blank>:0' --add_symbol '<unk>:1'")
    p.add_argument("--log_level", type=lambda x: x.upper(), default="INFO")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    logging.basicConfig(level=args.log_level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    if args.token_type != "phn":
        raise ValueError(f"--token_type {args.token_type}: the character and word modes are not implemented (phn)")
    if args.cleaner is not None:
        raise ValueError(f"--cleaner {args.cleaner}: text cleaners are not implemented (none)")
    if args.g2p is not None:
        raise ValueError(f"--g2p {args.g2p}: g2p is not implemented (the column holds phonemes already)")
    with open(args.csv, newline="", encoding="utf-8") as f:
        rows = [r[args.column] for r in csv.DictReader(f)]
    words = build_token_list(rows, args.add_symbol, args.cutoff)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        for w in words:
            f.write(w + "\n")
    logging.info(f"{len(words)} tokens -> {args.out}")


if __name__ == "__main__":
    main()
