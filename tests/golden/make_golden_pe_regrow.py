#!/usr/bin/env python3
"""Golden vectors of the positional table's regrowth, from the REAL reference (make_golden.REF).

    python tests/golden/make_golden_pe_regrow.py          (build container only; the reference never travels)

fs2_pe_regrow_small.npz: ONE reference FastSpeech2 object (FS2_SMALL, the weights of fs2_small.npz: seed 0) answers
  1. inference(u)                                                   -> a_*  (decoder table of length 5000)
  2. inference(long, durations, pitch, energy, use_teacher_forcing)   sum(durations) = long_t_feats > 5000: the decoder's
     LegacyRelPositionalEncoding regrows its table for good (positional_encoding.py:36-57); the 48-token text leaves the encoder's alone
  3. inference(u) again                                             -> b_*  (decoder table of length long_t_feats: other values)
Only the two short results and the long call's inputs are stored (the long output is ~1.7 MB); weights are rebuilt from
(name, shape, seed) by the tests.  The archive is written with fixed member timestamps, so a second run gives the same bytes.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from make_golden import ROOT, np_  # noqa: E402

sys.path.insert(0, ROOT)
from jatts_amd.synthetic import FS2_SMALL, synth_state_dict  # noqa: E402

OUT = os.path.join(HERE, "fs2_pe_regrow_small.npz")


def save_npz_deterministic(path, arrays):
    """np.savez_compressed with every member dated 1980-01-01 (numpy stamps the wall clock): byte-identical reruns."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(8)
    FastSpeech2 = G.import_reference()
    model = FastSpeech2(idim=20, **FS2_SMALL).eval()
    ref_sd = model.state_dict()
    model.load_state_dict(synth_state_dict(ref_sd, 0))
    g = torch.Generator().manual_seed(71)
    u = torch.randint(1, 20, (17,), generator=g)
    long_text = torch.randint(1, 20, (48,), generator=g)
    long_d = torch.randint(90, 130, (48,), generator=g)
    long_p = torch.randn(48, 1, generator=g)
    long_e = torch.randn(48, 1, generator=g)
    T_long = int(long_d.sum())
    assert 5000 < T_long < 6000, T_long
    out = {"keys": json.dumps([[k, list(v.shape)] for k, v in ref_sd.items()]), "u_text": np_(u),
           "long_text": np_(long_text), "long_durations": np_(long_d), "long_pitch": np_(long_p), "long_energy": np_(long_e),
           "long_t_feats": np.int64(T_long)}
    with torch.no_grad():
        a = model.inference(u)
        assert model.decoder.embed[-1].pe.size(1) == 5000
        r = model.inference(long_text, durations=long_d, pitch=long_p, energy=long_e, use_teacher_forcing=True)
        assert r["feat_gen"].shape[0] == T_long
        assert model.decoder.embed[-1].pe.size(1) == T_long and model.encoder.embed[-1].pe.size(1) == 5000
        b = model.inference(u)
    for p, rr in (("a", a), ("b", b)):
        for k in ("feat_gen", "duration", "pitch", "energy"):
            out[f"{p}_{k}"] = np_(rr[k])
    assert np.array_equal(out["a_duration"], out["b_duration"])
    print(f"T_long {T_long}; short frames {out['a_feat_gen'].shape[0]}; "
          f"max|a - b| feat_gen {float(np.abs(out['a_feat_gen'] - out['b_feat_gen']).max()):.3e}")
    save_npz_deterministic(OUT, out)
    print(os.path.basename(OUT), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
