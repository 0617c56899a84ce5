"""Stage 1 of the recipes on the GPU, one module per step (a CPU device or a missing library raises ``JattsHipError``):
  audio   ``read_audio`` with its sample-rate conversion as a kernel (``Resampler``)
  stft    the STFT front end (``Stft``), log-mel (``LogMelExtractor``) and ``Energy``
  pitch   ``Pitch``: autocorrelation F0 on the same front end, then the reference's steps after the raw track
  stats   ``FeatureStatistics`` and ``standardize``: StandardScaler as a running state on the device
  common  ``PackedWaves``, the batch the steps hand to each other, and the shared length-adjustment / token-average path
``jatts_amd.bin.preprocess`` and ``jatts_amd.bin.compute_statistics`` are the reference's stage-1 CLIs on top of them."""
from .audio import *  # noqa: F401,F403
from .common import PackedWaves, adjust_and_average, token_spans  # noqa: F401
from .pitch import *  # noqa: F401,F403
from .stats import *  # noqa: F401,F403
from .stft import *  # noqa: F401,F403
