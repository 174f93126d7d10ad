"""Container decoding, the one thing a loader worker does: WAV -> int16 PCM, JPEG / PNG -> uint8 RGB.  Host only; everything the
reference computes in floating point after `torchaudio.load` and `PIL.Image.open` runs on the device (vipant_amd/frontend.py
`pcm_wave`, `KaldiFbank`; vipant_amd/image_views.py)."""
from __future__ import annotations

import wave

import numpy as np

from ..errors import VipantError


def read_wav(path):
    """-> (int16 ndarray [n, ch], sample rate).  16-bit PCM only (the stdlib `wave` module reads nothing but PCM)."""
    try:
        with wave.open(str(path), "rb") as f:
            width, ch, rate, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
            raw = f.readframes(n) if width == 2 else b""
    except (wave.Error, EOFError) as e:
        raise VipantError(f"{path}: not a PCM WAV file ({e})") from e
    if width != 2:
        raise VipantError(f"{path}: {8 * width}-bit samples (sample width {width} bytes); only 16-bit PCM is read")
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16)          # (a copy: frombuffer's array is read-only)
    return pcm[:len(pcm) // ch * ch].reshape(-1, ch), int(rate)


def read_frame(path):
    """-> uint8 ndarray [h, w, 3]."""
    from PIL import Image
    with Image.open(str(path)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)
