"""Dataset statistics and normalisation (csrc/stats.hip): ``FeatureStatistics`` is the per-feature
``sklearn.preprocessing.StandardScaler`` of ``jatts/bin/compute_statistics.py:75-103`` as a running float64 state on the device
(``jatts_col_moments``: one launch pair per ``partial_fit``, fixed summation order, no read-back before ``finalize``), ``standardize`` the
``StandardScaler.transform`` of ``jatts/datasets/tts_dataset.py:69-145`` (``jatts_standardize``).  Pinned on sklearn 1.7.2
(``tests/golden/stats_kat.npz``).  ``python -m jatts_amd.bin.compute_statistics`` is the reference's CLI on top of them."""
import os

import numpy as np
import torch

from .. import _abi, hip
from .common import require_cuda, require_device_tensor

STATS_ROWS_PER_GROUP = _abi.STATS_ROWS_PER_GROUP      # rows per summation group of jatts_col_moments (the library's compile-time constant)


def stats_from_state(n, mean, m2):
    """(n, mean, M2) per column -> float64 ``(mean_, var_, scale_)`` as ``StandardScaler.partial_fit`` leaves them (sklearn 1.7.2,
    preprocessing/_data.py): var = M2 / n; scale = sqrt(var), except that a column which cannot be told from a constant one gets
    scale 1.0 -- ``_is_constant_feature``: var <= n eps var + (n mean eps)^2 with eps = float64's, the error bound of the two-pass
    variance; ``_handle_zeros_in_scale`` with that mask.  Pure numpy.  Raises ValueError for a non-finite state or an empty one."""
    n = np.atleast_1d(np.asarray(n, dtype=np.float64))
    mean = np.atleast_1d(np.asarray(mean, dtype=np.float64))
    m2 = np.atleast_1d(np.asarray(m2, dtype=np.float64))
    n = np.broadcast_to(n, mean.shape)
    if not (np.isfinite(n).all() and np.isfinite(mean).all() and np.isfinite(m2).all()):
        raise ValueError("statistics state is not finite (NaN or infinity in the features: they are not skipped)")
    if (n <= 0).any():
        raise ValueError("statistics of zero samples")
    var = m2 / n
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return mean.copy(), var, scale


_H5_ERROR = "{} .h5 stats needs h5py; convert to .npz (<feat>_mean, <feat>_scale)"


def save_stats(path, feat_name, mean, scale):
    """Write or update ``<feat_name>_mean`` / ``<feat_name>_scale`` (float32) in ``path`` (compute_statistics.py:94-103): .npz always
    (the twin format ``bin.tts_decode.read_stats`` reads; other entries of an existing file are kept), .h5 through h5py."""
    path = str(path)
    new = {f"{feat_name}_mean": np.asarray(mean).astype(np.float32), f"{feat_name}_scale": np.asarray(scale).astype(np.float32)}
    if path.endswith(".npz"):
        old = {}
        if os.path.exists(path):
            with np.load(path) as z:
                old = {k: z[k] for k in z.files}
        old.update(new)
        with open(path, "wb") as f:        # (np.savez appends ".npz" to a bare name; an open file is taken as it is)
            np.savez(f, **old)
        return
    try:
        import h5py
    except ImportError as e:
        raise ImportError(_H5_ERROR.format("writing")) from e
    with h5py.File(path, "a") as f:
        for k, v in new.items():
            if k in f:
                del f[k]
            f.create_dataset(k, data=v)


class FeatureStatistics:
    """One ``sklearn.preprocessing.StandardScaler`` of compute_statistics.py:81-92 as a running float64 state on the GPU.

    ``partial_fit`` / ``partial_fit_ragged`` / ``merge`` launch kernels and return; nothing is read back until ``finalize()``, the
    one synchronisation.  The state (``self.state``, float64 (3, dim): samples seen | mean | M2) is bit-identical from run to run for
    the same sequence of calls.  Unlike sklearn, NaN values are NOT skipped: they (and infinities) make ``finalize`` raise."""

    def __init__(self, dim, device="cuda"):
        self.dim = int(dim)
        if self.dim < 1:
            raise ValueError(f"dim {dim} must be positive")
        self.device = require_cuda(device)
        _abi.load()
        self.state = torch.zeros(3, self.dim, dtype=torch.float64, device=self.device)
        self._ws = torch.empty(2 * self.dim * 8, dtype=torch.float64, device=self.device)     # own scratch: grows, never shared

    def _fit(self, x, ld, rows):
        need = hip.col_moments_ws_doubles(rows, self.dim)
        if need > self._ws.numel():
            self._ws = torch.empty(2 * need, dtype=torch.float64, device=self.device)         # (stream-ordered: the old one may still be read)
        hip.col_moments(x, ld, self.dim, rows, self.state, self._ws)
        return self

    @torch.no_grad()
    def partial_fit(self, x, ld=None):
        """x: device f32 (rows, ld) with ld >= dim (columns dim.. are ignored), or (rows,) when dim == 1.  ``ld`` overrides the row
        pitch of a flat buffer."""
        require_device_tensor(x, "partial_fit takes a device tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"partial_fit: float32 expected, got {x.dtype}")
        if ld is None:
            if x.dim() == 1 and self.dim == 1:
                ld = 1
            elif x.dim() == 2:
                ld = x.shape[1]
            else:
                raise ValueError(f"partial_fit: (rows, ld) expected, got {tuple(x.shape)}")
        ld = int(ld)
        if ld < self.dim or x.numel() % ld:
            raise ValueError(f"partial_fit: {tuple(x.shape)} is not (rows, ld = {ld}) with ld >= dim = {self.dim}")
        return self._fit(x.contiguous(), ld, x.numel() // ld)

    def partial_fit_ragged(self, rb, feats):
        """What ``LogMelExtractor.__call__`` returns: the packed rows of all utterances of the batch are ONE partial_fit call."""
        if feats.dim() != 2 or feats.shape[0] != rb.total:
            raise ValueError("partial_fit_ragged: feats must hold the batch's packed rows")
        return self.partial_fit(feats)

    @torch.no_grad()
    def merge(self, other):
        """Fold another accumulator (a shard of the same dataset) into this one; ``other`` is left as it is."""
        if not isinstance(other, FeatureStatistics) or other.dim != self.dim or other is self:
            raise ValueError("merge: another FeatureStatistics of the same dim expected")
        hip.col_moments_merge(self.state, other.state.to(self.device))
        return self

    def finalize(self):
        """The one synchronisation: float64 numpy ``mean_``, ``var_``, ``scale_`` (dim,) and ``n_samples_seen_`` (int) as attributes
        and as the returned tuple.  ValueError when the state is not finite or empty."""
        st = self.state.cpu().numpy()
        self.mean_, self.var_, self.scale_ = stats_from_state(st[0], st[1], st[2])
        self.n_samples_seen_ = int(st[0][0])
        return self.mean_, self.var_, self.scale_, self.n_samples_seen_

    def save(self, path, feat_name):
        """finalize() and write ``<feat_name>_mean`` / ``<feat_name>_scale`` as float32 (see ``save_stats``)."""
        mean, _, scale, _ = self.finalize()
        save_stats(path, feat_name, mean, scale)


@torch.no_grad()
def standardize(x, mean, scale, dim=None):
    """``StandardScaler.transform`` (tts_dataset.py:69-145) on the GPU: device f32 x (rows, ld) -> (x - mean) / scale on the first
    ``dim`` columns (default: len(mean)), one f32 subtract and one f32 divide, both correctly rounded; columns dim.. are zero.
    ``mean`` / ``scale``: numpy or tensors, cast to float32 as the stats file stores them."""
    require_device_tensor(x, "standardize takes a device tensor")
    m = torch.as_tensor(np.asarray(mean, dtype=np.float32) if not isinstance(mean, torch.Tensor) else mean).to(torch.float32).reshape(-1)
    s = torch.as_tensor(np.asarray(scale, dtype=np.float32) if not isinstance(scale, torch.Tensor) else scale).to(torch.float32).reshape(-1)
    dim = int(m.numel()) if dim is None else int(dim)
    if m.numel() != s.numel() or not 1 <= dim <= m.numel():
        raise ValueError("standardize: mean and scale must have the same length >= dim")
    x2 = x.reshape(-1, 1) if x.dim() == 1 else x
    if x2.dim() != 2 or x2.shape[1] < dim or x2.dtype != torch.float32:
        raise ValueError(f"standardize: float32 (rows, ld >= {dim}) expected, got {x.dtype} {tuple(x.shape)}")
    y = hip.standardize(x2.contiguous(), m.to(x.device).contiguous(), s.to(x.device).contiguous(), dim)
    return y.reshape(-1) if x.dim() == 1 else y
