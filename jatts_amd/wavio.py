"""PCM wav decoding shared by the speaker-embedding front end (``spkemb.load_wav``) and stage 1 (``features.read_audio``): the stdlib
``wave`` module and numpy only (soundfile / torchaudio are absent from the build environment)."""
import wave

import numpy as np


def decode_wav(path):
    """-> (float32 ndarray (n_frames, n_channels) in [-1, 1), sampling rate): integer PCM of 8 (unsigned), 16, 24 or 32 bits divided
    by its full scale, the contract of torchaudio.load / soundfile.read for such files."""
    with wave.open(path, "rb") as w:
        sw, raw = w.getsampwidth(), w.readframes(w.getnframes())
        if sw == 2:
            a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
        elif sw == 4:
            a = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
        elif sw == 3:                                          # 24-bit: sign-extend the three little-endian bytes
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            a = ((v ^ 0x800000) - 0x800000).astype(np.float32) / 8388608.0
        elif sw == 1:                                          # 8-bit wav is unsigned
            a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        else:
            raise NotImplementedError(f"PCM wav with {8 * sw}-bit samples")
        return a.reshape(-1, w.getnchannels()), w.getframerate()
