from .hifigan import HiFiGANGenerator  # noqa: F401
from .vocoder import Vocoder  # noqa: F401
from .griffin_lim import GriffinLim, Spectrogram2Waveform  # noqa: F401
