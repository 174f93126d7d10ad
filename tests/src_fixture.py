"""A directory in the layout of the reference's raw-file image-audio dataset, generated into a temporary path: 16-bit WAVs written
with the stdlib `wave` module, PNG frames (lossless) written with PIL, and `{name}.csv` indices of one JSON record per line.  Shared
by tests/test_src_dataset_cpu.py and tests/test_src_trainer_gpu.py."""
import json
import os
import wave

import numpy as np

SR = 16000


def write_wav(path, pcm, rate=SR, width=2):
    """pcm int16 [n, ch] (width 2), or raw bytes of `width`-byte samples with `ch` given as pcm = (bytes, ch)."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        if isinstance(pcm, tuple):
            raw, ch = pcm
        else:
            raw, ch = np.ascontiguousarray(pcm.astype("<i2")).tobytes(), pcm.shape[1]
        f.setnchannels(ch)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw)


def write_png(path, frame):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(frame).save(path)


def noise_clip(g, n, ch, amp=6000):
    """Stationary noise with a little tone: the centred crop of such a clip keeps its standard deviation."""
    t = np.arange(n)[:, None]
    x = amp * g.standard_normal((n, ch)) + 0.3 * amp * np.sin(2 * np.pi * 440.0 * t / SR + np.arange(ch)[None, :])
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def make_src_dir(root, name, seconds, channels, frame_hw, nframes_per_item=None, sub_dirs=None, seed=3, clip_key="clip", prefix="c"):
    """Writes len(seconds) items and `{root}/{name}.csv` -> the records, the clips (int16 [n, ch]) and the frames (lists of uint8
    [h, w, 3], one per frame name) as written."""
    g = np.random.default_rng(seed)
    records, clips, frames = [], [], []
    for i, (sec, ch, hw) in enumerate(zip(seconds, channels, frame_hw)):
        ident = f"{prefix}{i}"
        sub = sub_dirs[i] if sub_dirs else ""
        base = f"{root}/{sub + '/' if sub else ''}"
        pcm = noise_clip(g, int(round(sec * SR)), ch)
        write_wav(f"{base}{clip_key}/{ident}.wav", pcm)
        k = nframes_per_item[i] if nframes_per_item else 0
        names = "png" if k == 0 else [f"{j:03d}.png" for j in range(k)]
        mine = []
        for fname in ([names] if k == 0 else names):
            fr = g.integers(0, 256, size=(hw[0], hw[1], 3), dtype=np.int64).astype(np.uint8)
            write_png(f"{base}frame/{ident}.{fname}", fr)
            mine.append(fr)
        records.append({"id": ident, "dir": sub, clip_key: ["wav"], "frame": names, "labels": [f"/m/{i % 3}"]})
        clips.append(pcm)
        frames.append(mine)
    with open(f"{root}/{name}.csv", "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    return records, clips, frames
