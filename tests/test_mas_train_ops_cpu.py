"""CPU: the MAS trainers' new entries are declared, bound and exported; autograd.GaussianUpsample differentiates hs only."""
import os
import re

import torch

from conftest import ROOT

NEW = ("jatts_gaussian_upsample_fwd", "jatts_gaussian_upsample_bwd", "jatts_alignment_logp_bwd")


def test_new_symbols_in_header_prototypes_and_library(lib):
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
        n_args = len(re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S).group(1).split(","))
        assert n_args == len(_abi.PROTOTYPES[name][1]), name
    assert _abi.ABI_VERSION == 8 and lib.jatts_abi_version() == 8       # these symbols were additive (no bump); 8 came with jatts_scratch


def test_gaussian_upsample_differentiates_hs_only(monkeypatch):
    from jatts_amd import autograd as A
    from jatts_amd import hip
    assert issubclass(A.GaussianUpsample, torch.autograd.Function)
    seen = {}

    def fake_bwd(ds, stat, g, kv, kvo, B, Tm, To, delta=0.1):
        seen["args"] = (ds, stat, B, Tm, To, delta)
        return torch.full((B * Tm, g.shape[1]), 2.0)

    monkeypatch.setattr(hip, "gaussian_upsample_bwd", fake_bwd)

    class Ctx:
        saved_tensors = (torch.ones(2, 3), torch.zeros(2 * 5, 2), torch.tensor([3, 2], dtype=torch.int32), torch.tensor([5, 4], dtype=torch.int32))
        geom = (2, 3, 5, 0.1)

    grads = A.GaussianUpsample.backward(Ctx, torch.ones(2 * 5, 4))
    assert len(grads) == 8 and grads[0].shape == (2 * 3, 4) and all(v is None for v in grads[1:])
    assert seen["args"][0] is Ctx.saved_tensors[0] and seen["args"][1] is Ctx.saved_tensors[1]      # ds and stat are what is saved, never p
