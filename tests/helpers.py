"""Shared test helpers: rebuild the golden models' weights from (name, shape, seed)."""
import json
import os
import sys

import numpy as np
import torch

from jatts_amd.synthetic import synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    keys = json.loads(str(z["keys"])) if "keys" in z.files else None
    return z, keys


def golden_state(keys, seed):
    return synth_state_dict({k: tuple(s) for k, s in keys}, seed)


def maxdiff(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) if a.numel() else 0.0


# The golden vectors were captured on an AVX-512 Intel host, where ATen, MKL and oneDNN run their AVX-512 kernels; on such a CPU the oracles
# reproduce them within the bounds the tests state (bit for bit at the bench length).  Where those libraries take narrower vector paths
# (another vendor, no AVX-512, or a path forced by environment) they sum f32 in another order: forcing the AVX2 and SSE paths on the capture
# host moves the oracle outputs by up to 6.5e-5 of their magnitude, so there the bound is REORDER_RTOL x max|ref| when that is larger.
REORDER_RTOL = 2e-4


def _on_capture_paths():
    if any(os.environ.get(k) for k in ("ATEN_CPU_CAPABILITY", "MKL_ENABLE_INSTRUCTIONS", "MKL_CBWR", "MKL_DEBUG_CPU_TYPE", "DNNL_MAX_CPU_ISA",
                                       "ONEDNN_MAX_CPU_ISA")):
        return False
    try:
        intel = any(ln.startswith("vendor_id") and "GenuineIntel" in ln for ln in open("/proc/cpuinfo"))
    except OSError:
        intel = False
    return intel and torch.backends.cpu.get_cpu_capability() == "AVX512"


ON_CAPTURE_PATHS = _on_capture_paths()


def golden_bound(tol, ref):
    """The bound an oracle output is held to against the golden vector `ref`: `tol` on the capture host's kernel paths, else the f32
    reordering bound where that is larger (see REORDER_RTOL)."""
    if ON_CAPTURE_PATHS:
        return tol
    return max(tol, REORDER_RTOL * float(np.abs(np.asarray(ref, dtype=np.float64)).max()))


def relerr(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / (b.norm() + 1e-30))


def hifigan_xcheck_case(name):
    """(params, state dict as the fixture's generator loaded it, mel, fixture) of one tests/golden/hifigan_xcheck.npz case: weights rebuilt
    from their seed (make_golden_hifigan_xcheck.py), `wn` as weight-norm (g, v) pairs."""
    from jatts_amd.synthetic import synth_hifigan_state
    z = np.load(os.path.join(GOLDEN, "hifigan_xcheck.npz"))
    params, wseed, frames, mseed = json.loads(str(z["cases"]))[name]
    params = {k: (tuple(tuple(d) if isinstance(d, list) else d for d in v) if isinstance(v, list) else v) for k, v in params.items()}
    sd = synth_hifigan_state(params, seed=wseed)
    if name == "wn":
        sys.path.insert(0, GOLDEN)
        from make_golden_hifigan_xcheck import wn_pairs
        sd, _ = wn_pairs(sd, wseed)
    mel = torch.tensor(z[f"{name}_mel"])
    assert mel.shape[0] == frames and torch.equal(mel, torch.randn(frames, params["in_channels"], generator=torch.Generator().manual_seed(mseed)))
    return params, sd, mel, z
