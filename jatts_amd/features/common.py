"""What the stage-1 steps share: the GPU-only refusals, the packed waveform batch they pass to each other (``PackedWaves``) and the path after
a per-frame track, length adjustment and token average (``adjust_and_average``; ``feature_extract/energy.py:88-122``, ``dio.py:128-159``)."""
import numpy as np
import torch

from .. import _abi, hip


def require_cuda(device, who="jatts_amd.features"):
    """-> torch.device; JattsHipError for anything but a GPU."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _abi.JattsHipError(f"{who} runs on the GPU only (no CPU fallback)")
    return device


def require_device_tensor(x, takes):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _abi.JattsHipError(f"jatts_amd.features runs on the GPU only (no CPU fallback): {takes}")


class PackedWaves:
    """A ragged batch of waveforms in one device buffer: ``x`` f32 (sum(lens),), ``lens`` on the host, ``cu`` their exclusive scan on the
    device (``cu_host`` on the host).  The one place waveforms are packed: what ``Resampler`` returns and every extractor consumes."""

    def __init__(self, x, lens):
        require_device_tensor(x, "PackedWaves takes a device tensor")
        self.lens = [int(v) for v in lens]
        if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.numel() != sum(self.lens) or min(self.lens, default=0) < 0:
            raise ValueError("PackedWaves: a contiguous 1-D float32 buffer of sum(lens) samples expected")
        self.x = x
        self.cu_host = hip.exclusive_scan(self.lens)
        self.cu = hip.h2d(self.cu_host, torch.int32, x.device)

    @classmethod
    def from_list(cls, waves, device):
        """numpy arrays, CPU tensors or device tensors of any shape -> one float32 buffer on ``device``; a PackedWaves is passed through."""
        if isinstance(waves, cls):
            return waves
        ws = [torch.as_tensor(w).reshape(-1).to(torch.float32) for w in waves]
        if not ws:
            raise ValueError("no waveform")
        return cls(torch.cat(ws).to(device).contiguous(), [int(w.numel()) for w in ws])

    def split(self):
        """list of per-utterance views of ``x``"""
        return [self.x[a:b] for a, b in zip(self.cu_host[:-1], self.cu_host[1:])]

    def select(self, indices):
        """A new PackedWaves of these utterances in this order (a copy): what packing them directly gives."""
        views = self.split()
        return PackedWaves(torch.cat([views[i] for i in indices]).contiguous(), [self.lens[i] for i in indices])


def token_spans(durations, frame_lens, reduction_factor=1):
    """One integer sequence of token durations per utterance -> (tokens per utterance, the concatenated per-utterance inclusive scans of
    durations * reduction_factor).  They must cover the utterance's frames up to a remainder below the factor (energy.py:104, dio.py:149)."""
    if len(durations) != len(frame_lens):
        raise ValueError("durations: one sequence per utterance")
    token_lens, cum = [], []
    for d, n in zip(durations, frame_lens):
        d = np.asarray(torch.as_tensor(d).cpu()).astype(np.int64).reshape(-1) * int(reduction_factor)
        if (d < 0).any() or not 0 <= n - int(d.sum()) < reduction_factor:
            raise ValueError(f"durations sum to {int(d.sum())}, the utterance has {n} frames")
        token_lens.append(d.size)
        cum.extend(int(v) for v in np.cumsum(d))
    return token_lens, cum


def adjust_and_average(rb, v, feat_lengths=None, durations=None, reduction_factor=1):
    """A per-frame track ``v`` f32 (rb.total,) -> list of per-utterance f32 device tensors.  ``feat_lengths``: truncate / zero-pad to these
    frame counts (jatts_energy_adjust); ``durations`` (see ``token_spans``): mean of the positive values per token (jatts_token_average)."""
    if feat_lengths is not None:
        if len(feat_lengths) != rb.n_seq or min(int(n) for n in feat_lengths) < 0:
            raise ValueError("feat_lengths: one non-negative length per utterance")
        rb_out = hip.RaggedBatch(feat_lengths, rb.device)
        v, rb = hip.energy_adjust(rb, rb_out, v), rb_out
    if durations is not None:
        token_lens, cum = token_spans(durations, rb.lens, reduction_factor)
        rb_tok = hip.RaggedBatch(token_lens, rb.device)
        v, rb = hip.token_average(rb_tok, rb, hip.h2d(cum or [0], torch.int32, rb.device), v), rb_tok
    return [v[a:b] for a, b in zip(rb.cu_host[:-1], rb.cu_host[1:])]
